"""fp64 numpy twin of the diagonally scaled preconditioner of the variable-density solve (the *_scaled entry points of
poisson_cnn_amd/csrc/varcoef.hip); tests/varcoef_twin.py and tests/varcoef_bc_twin.py hold the system and the plain loop.

Concus and Golub's scaling: z = s o M^-1 (s o r) with s = d^-1/2, d = diag(A) / diag(M) and M the constant-coefficient operator of the same edge
closure.  diag(M) is 4 / dx^2 at every unknown (beyond a Neumann edge the inward face counts twice in M as in A), so d is the mean of the node's four
face coefficients, the inward one taken twice on a Neumann edge.  diag(s) commutes with the trapezoid weights: s M^-1 s is self-adjoint in the W inner
product as M^-1 is, and with c the coefficients of s o r in M's eigenbasis, sum w r z = sum c^2 / (lam_h + lam_w)."""
import numpy as np

from tests import varcoef_bc_twin as B
from tests import varcoef_twin as T


def smooth_fixture(H, W, ratio, N=1):
    """N samples of the smooth fixture: rho = smooth_density(default_rng(0), ..) with min 1 and max `ratio` (further samples: further draws of the same
    generator), a random right-hand side and edge arrays, one spacing each -> (rho (N,H,W), f (N,H,W), edges dict of (N,len), dx (N,)), all fp32 values."""
    rng = np.random.default_rng(0)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    rho = f32(np.stack([T.smooth_density(rng, H, W, 1.0, ratio) for _ in range(N)]))
    f = f32(rng.uniform(-1, 1, (N, H, W)))
    e = {k: f32(rng.uniform(-1, 1, (N, W if k in ('left', 'right') else H))) for k in B.EDGES}
    return rho, f, e, f32(rng.uniform(5e-3, 5e-2, N))


def plain_pcg(A, b, H, W, mask, **kw):
    """The unscaled loop -> (x, iterations, relative residual): the all-Dirichlet twin's for mask 0, the per-edge twin's otherwise."""
    return T.pcg(A, b, (H - 2, W - 2), **kw) if mask == 0 else B.pcg(A, b, H, W, mask, **kw)


def scaling(A, dx):
    """s (mh mw,) = (diag(A) dx^2 / 4)^-1/2."""
    return 1.0 / np.sqrt(A.diagonal() * float(dx) ** 2 / 4.0)


def spectral(H, W, mask):
    """t (mh mw,) -> (M^-1 t with the lam = 0 mode dropped, sum c^2 / (lam_h + lam_w)): what the device's division pass produces."""
    nl, nr, nb, nt = B.flags(mask)
    Vih, Vh, lh, _ = B.axis_basis(H, nl, nr)
    Viw, Vw, lw, _ = B.axis_basis(W, nb, nt)
    lam = lh[:, None] + lw[None, :]
    keep = np.abs(lam) > 1e-13
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)

    def apply(t):
        c = Vih @ t.reshape(len(lh), len(lw)) @ Viw.T
        return (Vh @ (c * inv) @ Vw.T).ravel(), float((c * c * inv).sum())
    return apply


def pcg(A, b, H, W, mask, dx, tol=1e-10, max_iterations=500, x0=None, trace=None):
    """The scaled device loop, PCG in the W inner product (mask 0: every weight 1, the all-Dirichlet loop) -> (x, iterations, relative residual).
    r.z is the spectral sum, as on the device; trace, a list, receives (spectral sum, direct sum w r z) of every preconditioner application."""
    w = B.weights(H, W, mask).ravel()
    if mask == 15:
        b = B.project(b, B.weights(H, W, mask))[0]
    dot = lambda a, c: float(w @ (a * c))
    s, minv = scaling(A, dx), spectral(H, W, mask)

    def precondition(r):
        zt, rz = minv(s * r)
        z = s * zt
        if trace is not None:
            trace.append((rz, dot(r, z)))
        return z, rz

    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x
    bb = dot(b, b)
    it = 0
    if dot(r, r) > tol * tol * bb:
        z, rz = precondition(r)
        p = z.copy()
        while it < max_iterations:
            q = A @ p
            alpha = rz / dot(p, q)
            x += alpha * p
            r -= alpha * q
            it += 1
            if dot(r, r) <= tol * tol * bb:
                break
            z, rz_new = precondition(r)
            p = z + (rz_new / rz) * p
            rz = rz_new
    if mask == 15:
        x = x - float(w @ x) / float(w.sum())
    return x, it, (np.sqrt(dot(r, r) / bb) if bb > 0 else 0.0)
