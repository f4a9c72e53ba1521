"""Twin of pcnn_error_stats and pcnn_varcoef_error_stats (csrc/error_stats.hip): the same eight per-sample statistics in numpy float64 - or, with
float32_terms=True, every term (e, r, f) formed in float32 in the operation order the kernel documents and only the sums carried in float64, which
is what the kernel's sums are compared against.  Without rho the residual is the 5-point one, with rho the flux-form one."""
import numpy as np


def _field(a, N, H, W, dtype):
    return np.asarray(a, dtype=dtype).reshape(N, H, W)


def _pred(pred, dtype):
    p = np.asarray(pred, dtype=dtype)
    if p.ndim == 4:                                   # (N,1,H,W) or (N,H,W,1)
        p = p[:, 0] if p.shape[1] == 1 else p[..., 0]
    return p


def five_point_residual(pred, rhs, dx, dtype=np.float64):
    """r on the (H-2)(W-2) interior of every sample: the 3 x 3 second-order FD Laplacian of pred minus rhs; dx (N, 2), column 0 the H axis."""
    p = _pred(pred, dtype)
    N, H, W = p.shape
    f = _field(rhs, N, H, W, dtype)[:, 1:-1, 1:-1]
    d = np.asarray(dx, dtype=dtype).reshape(N, 2)
    one, two = dtype(1), dtype(2)
    ay, ax = (one / (d[:, 0] * d[:, 0]))[:, None, None], (one / (d[:, 1] * d[:, 1]))[:, None, None]
    c = p[:, 1:-1, 1:-1]
    return (p[:, :-2, 1:-1] - two * c + p[:, 2:, 1:-1]) * ay + (p[:, 1:-1, :-2] - two * c + p[:, 1:-1, 2:]) * ax - f


def residual(pred, rho, rhs, dx, dtype=np.float64):
    """The flux-form r on the (H-2)(W-2) interior of every sample, all arithmetic in `dtype`, in the kernel's order (index 0..3: towards i-1, i+1,
    j-1, j+1); dx (N,):  b_k = 2 / (rc + r_k), d_k = u_k - uc, s = (b_0 d_0 + b_1 d_1) + (b_2 d_2 + b_3 d_3), r = s * (1 / (dx dx)) - f."""
    p = _pred(pred, dtype)
    N, H, W = p.shape
    d, f = _field(rho, N, H, W, dtype), _field(rhs, N, H, W, dtype)[:, 1:-1, 1:-1]
    h = np.asarray(dx, dtype=dtype).reshape(N)
    two, one = dtype(2), dtype(1)
    inv_h2 = (one / (h * h))[:, None, None]
    uc, rc = p[:, 1:-1, 1:-1], d[:, 1:-1, 1:-1]
    nb = lambda a: (a[:, :-2, 1:-1], a[:, 2:, 1:-1], a[:, 1:-1, :-2], a[:, 1:-1, 2:])
    t = [(two / (rc + rk)) * (uk - uc) for uk, rk in zip(nb(p), nb(d))]
    r = ((t[0] + t[1]) + (t[2] + t[3])) * inv_h2 - f
    assert r.dtype == dtype
    return r


def error_stats(pred, target=None, rhs=None, dx=None, rho=None, float32_terms=False):
    """pred: (N, H, W), (N, 1, H, W) or (N, H, W, 1); target / rho / rhs: the same points; dx (N, 2) without rho, (N,) one spacing per sample with it.
    -> (N, 8) float64 {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}."""
    dtype = np.float32 if float32_terms else np.float64
    p = _pred(pred, dtype)
    N, H, W = p.shape
    out = np.zeros((N, 8))
    if target is not None:
        t = _field(target, N, H, W, dtype)
        e = (p - t).astype(np.float64)
        t = t.astype(np.float64)
        out[:, 0] = np.abs(e).sum(axis=(1, 2))
        out[:, 1] = (e * e).sum(axis=(1, 2))
        out[:, 2] = np.abs(e).max(axis=(1, 2))
        out[:, 3] = (t * t).sum(axis=(1, 2))
        out[:, 4] = np.abs(t).max(axis=(1, 2))
    if rhs is not None:
        if dx is None:
            raise ValueError('rhs needs dx')
        if H < 3 or W < 3:
            raise ValueError('the residual needs H, W >= 3')
        r = (five_point_residual(p, rhs, dx, dtype) if rho is None else residual(p, rho, rhs, dx, dtype)).astype(np.float64)
        f = _field(rhs, N, H, W, np.float64)[:, 1:-1, 1:-1]
        out[:, 5] = (r * r).sum(axis=(1, 2))
        out[:, 6] = np.abs(r).max(axis=(1, 2))
        out[:, 7] = (f * f).sum(axis=(1, 2))
    return out
