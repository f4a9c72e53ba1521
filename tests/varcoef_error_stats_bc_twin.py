"""Twin of pcnn_varcoef_bc_error_stats (csrc/error_stats.hip): the eight per-sample statistics of a prediction of the
variable-density problem with per-edge Dirichlet / Neumann boundaries, in numpy.  Columns 0..4 are tests/error_stats_twin.py's.  The residual columns
run over the unknowns of the mask (varcoef_bc_twin.unknowns) with w = varcoef_bc_twin.weights:  sum w r^2, max|r|, sum w f^2.

float64 (the default): r = varcoef_train_bc_twin.residual, b - A x of the assembled system with the field's own Dirichlet edge values and du/dn = 0.
float32_terms=True: every term formed in float32 in the operation order of pcnn_flux_residual (csrc/flux_form.h), only the sums carried in float64,
as tests/error_stats_twin.py does for mask 0 - what the kernel's numbers are compared against.  That order is `ordered_residual`, which reads the
neighbour beyond a Neumann edge at the mirrored index, as the kernel does; in float64 it is a second statement of the same r."""
import numpy as np

from tests import error_stats_twin as TW, varcoef_bc_twin as B, varcoef_train_bc_twin as BT


def _mirrored(a, mask):
    """(H,W) -> (H+2,W+2): beyond a Neumann edge the mirror image (node 1 / n-2); beyond a Dirichlet edge nothing an unknown reads (NaN)."""
    H, W = a.shape
    nl, nr, nb, nt = B.flags(mask)
    out = np.full((H + 2, W + 2), np.nan, dtype=a.dtype)
    out[1:-1, 1:-1] = a
    if nl:
        out[0, 1:-1] = a[1]
    if nr:
        out[-1, 1:-1] = a[-2]
    if nb:
        out[1:-1, 0] = a[:, 1]
    if nt:
        out[1:-1, -1] = a[:, -2]
    return out


def ordered_residual(pred, rho, rhs, dx, mask, dtype=np.float64):
    """One sample, (mh, mw): r on the unknowns, all arithmetic in `dtype` in the kernel's order (index 0..3: towards i-1, i+1, j-1, j+1):
    b_k = 2 / (rc + r_k), d_k = u_k - uc, s = (b_0 d_0 + b_1 d_1) + (b_2 d_2 + b_3 d_3), r = s * (1 / (dx dx)) - f."""
    p, d, f = (np.asarray(a, dtype=dtype) for a in (pred, rho, rhs))
    H, W = p.shape
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    P, D = _mirrored(p, mask), _mirrored(d, mask)
    si, sj = slice(i0 + 1, i1 + 2), slice(j0 + 1, j1 + 2)                       # the unknowns inside the padded arrays
    sh = lambda a, di, dj: a[si.start + di:si.stop + di, sj.start + dj:sj.stop + dj]
    two, one = dtype(2), dtype(1)
    h = dtype(dx)
    inv_h2 = one / (h * h)
    uc, rc = P[si, sj], D[si, sj]
    t = [(two / (rc + sh(D, di, dj))) * (sh(P, di, dj) - uc) for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1))]
    r = ((t[0] + t[1]) + (t[2] + t[3])) * inv_h2 - f[i0:i1 + 1, j0:j1 + 1]
    assert r.dtype == dtype and np.all(np.isfinite(r))
    return r


def error_stats(pred, rho=None, target=None, rhs=None, dx=None, mask=0, float32_terms=False):
    """pred / target / rho / rhs: (N,H,W) (or pred (N,1,H,W) / (N,H,W,1)); dx (N,).  -> (N, 8) float64."""
    dtype = np.float32 if float32_terms else np.float64
    p = TW._pred(pred, dtype)
    N, H, W = p.shape
    out = TW.error_stats(p, target, float32_terms=float32_terms)             # columns 0..4; 5..7 stay 0 without rhs
    if rhs is None:
        return out
    if dx is None or rho is None:
        raise ValueError('rhs needs rho and dx')
    if H < 3 or W < 3:
        raise ValueError('the residual needs H, W >= 3')
    d, f = TW._field(rho, N, H, W, dtype), TW._field(rhs, N, H, W, dtype)
    h = np.asarray(dx, dtype=dtype).reshape(N)
    w = B.weights(H, W, mask)
    si, sj = BT.unknown_slices(H, W, mask)
    for n in range(N):
        if float32_terms:
            r = ordered_residual(p[n], d[n], f[n], h[n], mask, np.float32).astype(np.float64)
        else:
            r = BT.residual(p[n], d[n], f[n], float(h[n]), mask)
        fu = f[n][si, sj].astype(np.float64)
        out[n, 5] = (w * r * r).sum()
        out[n, 6] = np.abs(r).max()
        out[n, 7] = (w * fu * fu).sum()
    return out
