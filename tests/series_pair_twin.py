"""Twin of pcnn_series_pair_synthesis (include/pcnn.h) and of the edge-type -> basis map of reverse_poisson_dataset_generator_mixed, written from
their definitions in numpy.

  soln[n,a,b] = sum_{A,B} c[n,A,B] phi_A(x_a) psi_B(y_b)
  rhs[n,a,b]  = sum_{A,B} c[n,A,B] (lam_a[n,A] + lam_b[n,B]) phi_A(x_a) psi_B(y_b),      x = linspace(0, pi, H), y = linspace(0, pi, W)

with, for the mode A = 1..k of basis 0 / 1 / 2 / 3:  sin(A t) / cos(A t) / sin((A - 1/2) t) / cos((A - 1/2) t).

`pair(..., dtype=np.float64)` is the reference.  `pair(..., dtype=np.float32)` restates the same sums with EVERY intermediate rounded to float32 -
the grid step pi / (n - 1), the angle, the frequency times the angle, the trig value, every product and every partial sum (B first, then A) - so
its distance from the reference is what float32 arithmetic alone costs on given inputs; numpy has no fused multiply-add, so each product is
rounded before it is added."""
import numpy as np

EDGES = ('left', 'right', 'bottom', 'top')


def grid(n, dtype=np.float64):
    """linspace(0, pi, n); in float32 as index * (pi / (n - 1)) with both factors rounded."""
    if np.dtype(dtype) == np.float64:
        return np.linspace(0.0, np.pi, n)
    f = np.float32
    step = f(np.pi) / f(n - 1) if n > 1 else f(0)
    return np.arange(n, dtype=f) * step


def basis(kind, k, t, dtype=np.float64):
    """(k, len(t)) table of the modes 1..k of basis `kind` on the points t: the frequency first, then frequency * angle."""
    if kind not in (0, 1, 2, 3):
        raise ValueError('basis %r not in 0..3' % (kind,))
    f = np.dtype(dtype).type
    w = np.arange(1, k + 1).astype(dtype) - f(0.5 if kind & 2 else 0.0)
    arg = (w[:, None] * np.asarray(t, dtype=dtype)[None, :]).astype(dtype)
    return (np.cos(arg) if kind & 1 else np.sin(arg)).astype(dtype)


def pair(coef, lam_a, lam_b, H, W, basis_a, basis_b, dtype=np.float64):
    """coef (N,ka,kb), lam_a (N,ka), lam_b (N,kb) -> (soln, rhs), each (N,H,W), every intermediate in `dtype`; returned as float64."""
    c, la, lb = (np.asarray(v).astype(dtype) for v in (coef, lam_a, lam_b))
    N, ka, kb = c.shape
    F, P = basis(basis_a, ka, grid(H, dtype), dtype), basis(basis_b, kb, grid(W, dtype), dtype)          # (ka,H), (kb,W)
    soln, rhs = np.zeros((N, H, W), dtype=dtype), np.zeros((N, H, W), dtype=dtype)
    for n in range(N):
        T, Tp = np.zeros((ka, W), dtype=dtype), np.zeros((ka, W), dtype=dtype)
        for B in range(kb):
            T = T + c[n, :, B, None] * P[B][None, :]
            Tp = Tp + (c[n, :, B] * lb[n, B])[:, None] * P[B][None, :]
        G = la[n][:, None] * T + Tp
        for A in range(ka):
            soln[n] = soln[n] + F[A][:, None] * T[A][None, :]
            rhs[n] = rhs[n] + F[A][:, None] * G[A][None, :]
    assert soln.dtype == np.dtype(dtype) and rhs.dtype == np.dtype(dtype)
    return soln.astype(np.float64), rhs.astype(np.float64)


def neumann_flags(boundary_types):
    """dict edge -> 'dirichlet' | 'neumann' (missing: Dirichlet) -> (left, right, bottom, top) booleans."""
    return tuple(str((boundary_types or {}).get(e, 'dirichlet')).lower() == 'neumann' for e in EDGES)


def axis_basis(lo, hi):
    """(low end, high end) Neumann flags of one axis -> basis: (D,D) 0, (N,N) 1, (D,N) 2, (N,D) 3."""
    return {(False, False): 0, (True, True): 1, (False, True): 2, (True, False): 3}[(bool(lo), bool(hi))]


def bases_of(flags, ka, kb):
    """(left, right, bottom, top) -> (basis_a, basis_b, omega_a (ka,), omega_b (kb,)): left / right are the ends of axis -2, bottom / top of axis -1;
    omega = A for the whole-wave bases 0 and 1, A - 1/2 for the quarter-wave bases 2 and 3."""
    ba, bb = axis_basis(flags[0], flags[1]), axis_basis(flags[2], flags[3])
    wa = np.arange(1, ka + 1, dtype=np.float64) - (0.5 if ba & 2 else 0.0)
    wb = np.arange(1, kb + 1, dtype=np.float64) - (0.5 if bb & 2 else 0.0)
    return ba, bb, wa, wb


def eigenvalues(omega, dx, n):
    """lam = -(pi omega / L)^2 with L = dx * n per sample: omega (k,), dx (N,) -> (N,k)."""
    L = np.asarray(dx, dtype=np.float64) * n
    return -(np.pi * np.asarray(omega, dtype=np.float64)[None, :] / L[:, None]) ** 2


def all_flags():
    return [tuple(bool(m >> i & 1) for i in range(4)) for m in range(16)]


# ---- the properties of a pair u, f (N,H,W) float64 with spacings dx (N,)
def pde_residual(u, f, dx):
    """rel-L2 per sample of the 5-point Laplacian of u against f on the interior, at each axis' effective spacing dx n / (n - 1): the series live
    on linspace(0, pi, n) while L = dx n."""
    N, H, W = u.shape
    out = []
    for n in range(N):
        hy, hx = dx[n] * H / (H - 1), dx[n] * W / (W - 1)
        lap = (u[n, 2:, 1:-1] - 2 * u[n, 1:-1, 1:-1] + u[n, :-2, 1:-1]) / hy ** 2 + (u[n, 1:-1, 2:] - 2 * u[n, 1:-1, 1:-1] + u[n, 1:-1, :-2]) / hx ** 2
        r = f[n, 1:-1, 1:-1]
        out.append(np.linalg.norm(lap - r) / np.linalg.norm(r))
    return max(out)


def edge_slices(u):
    """edge -> (the edge's values, the next line in, the one after): axis -2 carries left / right, axis -1 bottom / top."""
    return {'left': (u[:, 0, :], u[:, 1, :], u[:, 2, :]), 'right': (u[:, -1, :], u[:, -2, :], u[:, -3, :]),
            'bottom': (u[:, :, 0], u[:, :, 1], u[:, :, 2]), 'top': (u[:, :, -1], u[:, :, -2], u[:, :, -3])}


def edge_defects(u, flags):
    """(largest |u| on a Dirichlet edge, largest |-3 u0 + 4 u1 - u2| on a Neumann edge), both relative to max|u|; 0 where there is no such edge."""
    d = n = 0.0
    for e, neu in zip(EDGES, flags):
        u0, u1, u2 = edge_slices(u)[e]
        if neu:
            n = max(n, float(np.abs(-3 * u0 + 4 * u1 - u2).max()))
        else:
            d = max(d, float(np.abs(u0).max()))
    m = float(np.abs(u).max())
    return d / m, n / m
