"""fp64 numpy twin of pcnn_varcoef_series_pair (include/pcnn.h): a series solution of the edge types' eigenfunction
families and the DISCRETE right-hand side of the variable-density flux form, without a solve.

    u[i,j] = sum_{A,B} c[A,B] phi_A(x_i) psi_B(y_j),  x = linspace(0, pi, H), y = linspace(0, pi, W)      (series_pair_twin's bases and map)
    f      = L_h(rho) u = sum_k m_k beta_k (u_k - u_c) / dx^2 on the unknowns of the mask, 0 elsewhere       (m = 2 on a Neumann edge node's inward face)

The operator is restated here by slices of mirrored paddings - NOT through the sparse A of tests/varcoef_bc_twin.py, which the tests compare it with
(f = -A u).  u is an exact 0 on a node that is not an unknown (the sine factor leaves 1e-16 there), as the kernel writes it."""
import numpy as np

from tests import series_pair_twin as SP, varcoef_bc_twin as B, varcoef_train_bc_twin as BT

EPS32 = float(np.finfo(np.float32).eps)


def series(coef, H, W, mask):
    """coef (ka,kb) -> u (H,W) float64, zero on the nodes that are not unknowns."""
    c = np.asarray(coef, dtype=np.float64)
    ba, bb, _, _ = SP.bases_of(B.flags(mask), c.shape[0], c.shape[1])
    F, P = SP.basis(ba, c.shape[0], SP.grid(H)), SP.basis(bb, c.shape[1], SP.grid(W))                   # (ka,H), (kb,W)
    u = np.zeros((H, W))
    si, sj = BT.unknown_slices(H, W, mask)
    u[si, sj] = (F.T @ c @ P)[si, sj]
    return u


def _padded(a, mask, fill):
    """(H+2, W+2): a with one more node on every side - beyond a Neumann edge the mirrored inward neighbour, else `fill`."""
    nl, nr, nb, nt = B.flags(mask)
    H, W = a.shape
    p = np.full((H + 2, W + 2), float(fill))
    p[1:-1, 1:-1] = a
    if nl:
        p[0, 1:-1] = a[1]
    if nr:
        p[-1, 1:-1] = a[-2]
    if nb:
        p[:, 0] = p[:, 2]
    if nt:
        p[:, -1] = p[:, -3]
    return p


def operator(u, rho, dx, mask):
    """L_h(rho) u on the unknowns of the mask, 0 elsewhere; u, rho (H,W)."""
    u, rho = np.asarray(u, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    H, W = u.shape
    up, rp = _padded(u, mask, 0.0), _padded(rho, mask, 1.0)
    uc, rc = up[1:-1, 1:-1], rp[1:-1, 1:-1]
    L = np.zeros((H, W))
    for sl in ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)), (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))):
        L += 2.0 / (rc + rp[sl]) * (up[sl] - uc)
    out = np.zeros((H, W))
    si, sj = BT.unknown_slices(H, W, mask)
    out[si, sj] = (L / float(dx) ** 2)[si, sj]
    return out


def twin(coef, rho, dx, mask):
    """coef (N,ka,kb), rho (N,H,W), dx (N,) -> (u64, f64), each (N,H,W) float64."""
    rho = np.asarray(rho, dtype=np.float64)
    N, H, W = rho.shape
    u = np.stack([series(coef[n], H, W, mask) for n in range(N)])
    f = np.stack([operator(u[n], rho[n], float(np.reshape(dx, -1)[n]), mask) for n in range(N)])
    return u, f


def trapezoid_weights(H, W):
    """The trapezoidal weights of the whole grid: 1/2 on every edge line - varcoef_bc_twin.weights(H, W, 15)."""
    return B.weights(H, W, 15)


# ----------------------------------------------------------------------------- fixtures shared by the reference and the GPU tests
SHAPES = ((33, 47), (45, 70), (97, 65))          # none a multiple of the 16 x 64 tile; one narrower than a tile; one more than a tile both ways
MODES = ((5, 8), (16, 16))
DX = (0.01, 0.02, 0.035)
RATIO = 1000.0


def coefficients(N, ka, kb, seed=0):
    return (2.0 * np.random.default_rng([seed, ka, kb]).uniform(size=(N, ka, kb)) - 1.0).astype(np.float32)


def smooth_unit_field(N, H, W, seed=1):
    """(N,H,W) float32 with max|g| = 1 per sample: a few random low modes, sign changes included - what varcoef_density turns into rho."""
    rng = np.random.default_rng([seed, H, W])
    x, y = np.linspace(0.0, 1.0, H)[:, None], np.linspace(0.0, 1.0, W)[None, :]
    g = np.zeros((N, H, W))
    for n in range(N):
        for a in range(4):
            for b in range(4):
                g[n] += rng.normal() / (1 + a + b) * np.cos(np.pi * a * x + rng.uniform(0, np.pi)) * np.cos(np.pi * b * y + rng.uniform(0, np.pi))
        g[n] /= np.abs(g[n]).max()
    return g.astype(np.float32)


def density(g, lo=1.0, hi=RATIO):
    """pcnn_varcoef_density in float32: lo + (hi - lo) min(|g|, 1)."""
    f = np.float32
    return (f(lo) + (f(hi) - f(lo)) * np.minimum(np.abs(g.astype(f)), f(1))).astype(f)


def zero_edges(H, W):
    return {'left': np.zeros(W), 'right': np.zeros(W), 'bottom': np.zeros(H), 'top': np.zeros(H)}


def round_trip(coef, rho, dx, mask):
    """What a perfect solver makes of the pair as the kernel stores it: the direct fp64 solve (varcoef_bc_twin.solve; mask 15: the projected system
    with zero trapezoidal mean) with float32(f64) as data, against float32(u64) - rel-L2 per sample.  The two roundings are all that separates them."""
    u, f = twin(coef, rho, dx, mask)
    N, H, W = u.shape
    out = []
    for n in range(N):
        back = B.solve(np.asarray(rho[n], dtype=np.float64), f[n].astype(np.float32).astype(np.float64), zero_edges(H, W), float(dx[n]), mask)
        out.append(BT.rel_l2(back, u[n].astype(np.float32)))
    return np.array(out)
