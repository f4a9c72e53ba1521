"""fp64 twin of pcnn_error_stats (csrc/error_stats.hip): the same eight per-sample statistics in numpy float64."""
import numpy as np


def error_stats(pred, target=None, rhs=None, dx=None):
    """pred: (N, H, W), (N, 1, H, W) or (N, H, W, 1); target / rhs: the same points; dx (N, 2), column 0 the H axis.
    -> (N, 8) float64 {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}."""
    p = np.asarray(pred, dtype=np.float64)
    if p.ndim == 4:                                   # (N,1,H,W) or (N,H,W,1)
        p = p[:, 0] if p.shape[1] == 1 else p[..., 0]
    N, H, W = p.shape
    out = np.zeros((N, 8))
    if target is not None:
        t = np.asarray(target, dtype=np.float64).reshape(N, H, W)
        e = p - t
        out[:, 0] = np.abs(e).sum(axis=(1, 2))
        out[:, 1] = (e * e).sum(axis=(1, 2))
        out[:, 2] = np.abs(e).max(axis=(1, 2))
        out[:, 3] = (t * t).sum(axis=(1, 2))
        out[:, 4] = np.abs(t).max(axis=(1, 2))
    if rhs is not None:
        if H < 3 or W < 3:
            raise ValueError('the residual needs H, W >= 3')
        f = np.asarray(rhs, dtype=np.float64).reshape(N, H, W)[:, 1:-1, 1:-1]
        d = np.asarray(dx, dtype=np.float64).reshape(N, 2)
        ay, ax = (1.0 / d[:, 0] ** 2)[:, None, None], (1.0 / d[:, 1] ** 2)[:, None, None]
        c = p[:, 1:-1, 1:-1]
        r = (p[:, :-2, 1:-1] - 2.0 * c + p[:, 2:, 1:-1]) * ay + (p[:, 1:-1, :-2] - 2.0 * c + p[:, 1:-1, 2:]) * ax - f
        out[:, 5] = (r * r).sum(axis=(1, 2))
        out[:, 6] = np.abs(r).max(axis=(1, 2))
        out[:, 7] = (f * f).sum(axis=(1, 2))
    return out
