"""ctypes wrappers of the dataset kernels of libpcnn (include/pcnn.h, "dataset" section)."""
import os
from ctypes import c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from .. import _lib, ops
from ..ops import _p, handle

_dst_cache = {}


def dst_matrices(n, device):
    """Device copies of the orthonormal DST-I matrix and eigenvalues for an n-point axis (cached per n: shapes change per batch)."""
    key = (n, str(device))
    if key not in _dst_cache:
        m = n - 2
        S = np.zeros((m, m), dtype=np.float64)
        lam = np.zeros(m, dtype=np.float64)
        rc = _lib.load().pcnn_dst_setup(c_int(n), S.ctypes.data_as(c_void_p), lam.ctypes.data_as(c_void_p))
        if rc != 0:
            raise RuntimeError('pcnn_dst_setup failed (%d)' % rc)
        _dst_cache[key] = (torch.tensor(S, device=device), torch.tensor(lam, device=device))
    return _dst_cache[key]


FFT_FROM = 2048          # solver='auto': rocFFT route from this many points per axis - measured crossover (profiles/r04_fd_solver_routes.txt: per sample
                         # 0.25 vs 0.35 ms at 1024^2, 0.80 vs 1.11 at 1536^2, 1.86 vs 1.66 at 2048^2; the odd extension has awkward lengths, 2046 = 2 3 11 31)


def fd_poisson_dst(rhs, left, right, bottom, top, dx, solver='auto'):
    """rhs (N,H,W); left/right (N,W); bottom/top (N,H); dx (N,) -> soln (N,H,W), all fp32 CUDA tensors.
    solver: 'gemm' (DST-I as fp64 matrix-core GEMMs, pcnn_fd_poisson_dst), 'fft' (rocFFT, pcnn_fd_poisson_fft) or 'auto' (fft from FFT_FROM
    points per axis; environment PCNN_FD_SOLVER overrides)."""
    N, H, W = rhs.shape
    Sh, lh = dst_matrices(H, rhs.device)
    Sw, lw = dst_matrices(W, rhs.device)
    solver = os.environ.get('PCNN_FD_SOLVER', solver)
    if solver not in ('auto', 'gemm', 'fft'):
        raise ValueError("solver must be 'auto', 'gemm' or 'fft'")
    if solver == 'fft' or (solver == 'auto' and min(H, W) >= FFT_FROM):
        ws = torch.empty((_lib.load().pcnn_fd_poisson_fft_workspace(c_int(N), c_int(H), c_int(W)) + 7) // 8, dtype=torch.float64, device=rhs.device)
        soln = torch.empty_like(rhs)
        handle().call('pcnn_fd_poisson_fft', c_int(N), c_int(H), c_int(W), _p(rhs), _p(left), _p(right), _p(bottom), _p(top), _p(dx), _p(lh), _p(lw), _p(ws), _p(soln))
        return soln
    tmp = torch.empty(2 * N * (H - 2) * (W - 2), dtype=torch.float64, device=rhs.device)
    soln = torch.empty_like(rhs)
    handle().call('pcnn_fd_poisson_dst', c_int(N), c_int(H), c_int(W), _p(rhs), _p(left), _p(right), _p(bottom), _p(top), _p(dx),
                  _p(Sh), _p(lh), _p(Sw), _p(lw), _p(tmp), _p(soln))
    return soln


_axis_cache = {}


def axis_decomposition(n, neumann_lo, neumann_hi, device):
    """Eigen-decomposition M = V diag(lam) V^-1 of the 1-D operator (2 on the diagonal, -1 beside it, the mirrored neighbour counted twice
    in a Neumann end's row) on the unknowns of an n-point axis: Dirichlet ends are not unknowns.  With W = diag(1/2 at Neumann ends, 1
    elsewhere) W M is symmetric, so the generalised symmetric problem (W M) v = lam W v gives V with V^T W V = I, i.e. V^-1 = V^T W (fp64,
    host, cached per (n, end types); Dirichlet-Dirichlet reproduces the DST-I basis of pcnn_dst_setup).
    Returns device tensors (Vinv, V, lam) and the index range (a, b) of the unknowns."""
    key = (n, bool(neumann_lo), bool(neumann_hi), str(device))
    if key not in _axis_cache:
        import scipy.linalg
        a, b = (0 if neumann_lo else 1), (n - 1 if neumann_hi else n - 2)
        m = b - a + 1
        M = 2.0 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)
        w = np.ones(m)
        if neumann_lo:
            M[0, 1] = -2.0
            w[0] = 0.5
        if neumann_hi:
            M[m - 1, m - 2] = -2.0
            w[m - 1] = 0.5
        Wm = np.diag(w)
        lam, V = scipy.linalg.eigh(Wm @ M, Wm)
        if neumann_lo and neumann_hi:
            lam[0] = 0.0                                        # exact null mode (constants)
        Vinv = V.T * w[None, :]
        # scipy hands V back in Fortran order and torch.tensor keeps those strides: the kernels read raw row-major memory
        _axis_cache[key] = (torch.tensor(np.ascontiguousarray(Vinv), device=device).contiguous(), torch.tensor(np.ascontiguousarray(V), device=device).contiguous(),
                            torch.tensor(np.ascontiguousarray(lam), device=device), (a, b))
    return _axis_cache[key]


def fd_poisson_mixed(rhs, left, right, bottom, top, dx, neumann=(False, False, False, False)):
    """5-point solve with per-edge Dirichlet / Neumann conditions; `neumann` = (left, right, bottom, top).  A Neumann edge's array holds
    du/dn (outward normal), a Dirichlet edge's its values.  rhs (N,H,W); left/right (N,W); bottom/top (N,H); dx (N,) -> soln (N,H,W)."""
    N, H, W = rhs.shape
    nl, nr, nb, nt = [bool(v) for v in neumann]
    Vih, Vh, lh, _ = axis_decomposition(H, nl, nr, rhs.device)
    Viw, Vw, lw, _ = axis_decomposition(W, nb, nt, rhs.device)
    mh, mw = Vh.shape[0], Vw.shape[0]
    key = ('T', W, nb, nt, str(rhs.device))
    if key not in _axis_cache:
        _axis_cache[key] = (Viw.t().contiguous(), Vw.t().contiguous())
    ViwT, VwT = _axis_cache[key]
    tmp = torch.empty(2 * N * mh * mw, dtype=torch.float64, device=rhs.device)
    soln = torch.empty_like(rhs)
    mask = int(nl) | (int(nr) << 1) | (int(nb) << 2) | (int(nt) << 3)
    handle().call('pcnn_fd_poisson_mixed', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rhs.contiguous()), _p(left.contiguous()), _p(right.contiguous()),
                  _p(bottom.contiguous()), _p(top.contiguous()), _p(dx.contiguous()), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(tmp), _p(soln))
    return soln


def _chk_varcoef(t, name, shape, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous CUDA %s tensor of shape %r' % (name, str(dtype).replace('torch.', ''), tuple(shape)))
    return t


def _neumann_mask(neumann):
    flags = [bool(v) for v in neumann]
    if len(flags) != 4:
        raise ValueError('neumann must be four flags (left, right, bottom, top), got %r' % (neumann,))
    return sum(int(v) << k for k, v in enumerate(flags))


def varcoef_unknowns(H, W, neumann):
    """Row range (i0, i1) and column range (j0, j1), both inclusive, of the unknowns for `neumann` = (left, right, bottom, top): a Neumann edge's
    nodes are unknowns, a Dirichlet edge's are not (fd_unknowns of csrc/pcnn_internal.h)."""
    nl, nr, nb, nt = [bool(v) for v in neumann]
    return (0 if nl else 1, H - 1 if nr else H - 2), (0 if nb else 1, W - 1 if nt else W - 2)


def varcoef_weights(H, W, neumann, device=None):
    """(w_i (mh,), w_j (mw,)) fp64: the axis weights of the W inner product of the solve with Neumann edges, 1/2 on a Neumann edge's row / column -
    the weights of axis_decomposition; w = w_i[:, None] * w_j[None, :]."""
    (i0, i1), (j0, j1) = varcoef_unknowns(H, W, neumann)
    wi, wj = torch.ones(i1 - i0 + 1, dtype=torch.float64, device=device), torch.ones(j1 - j0 + 1, dtype=torch.float64, device=device)
    for w, lo, hi in ((wi, neumann[0], neumann[1]), (wj, neumann[2], neumann[3])):
        if lo:
            w[0] = 0.5
        if hi:
            w[-1] = 0.5
    return wi, wj


def _varcoef_bases(H, W, neumann, device):
    """The six arrays (Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w) of the preconditioner.  An axis with two Dirichlet ends takes the DST-I matrix of
    dst_matrices for all of its matrices - the basis axis_decomposition reproduces for those ends, symmetric and its own inverse, and the one the
    all-Dirichlet entry points use, so mask 0 gives their bits; any other axis takes axis_decomposition's, cached like fd_poisson_mixed's."""
    nl, nr, nb, nt = [bool(v) for v in neumann]
    if nl or nr:
        Vih, Vh, lh, _ = axis_decomposition(H, nl, nr, device)
    else:
        Vh, lh = dst_matrices(H, device)
        Vih = Vh
    if nb or nt:
        Viw, Vw, lw, _ = axis_decomposition(W, nb, nt, device)
        key = ('T', W, nb, nt, str(device))
        if key not in _axis_cache:
            _axis_cache[key] = (Viw.t().contiguous(), Vw.t().contiguous())
        ViwT, VwT = _axis_cache[key]
    else:
        VwT, lw = dst_matrices(W, device)
        ViwT = VwT
    return Vih, Vh, lh, ViwT, VwT, lw


def varcoef_apply(rho, dx, p, neumann=None, reaction=None):
    """q = A p of the variable-density flux-form operator (include/pcnn.h, pcnn_varcoef_apply) with zero Dirichlet data, and the per-sample p.q
    of the same pass.  rho (N,H,W) fp32, dx (N,) fp32, p (N,H-2,W-2) fp64 -> q (N,H-2,W-2) fp64, pq (N,) fp64.
    neumann = (left, right, bottom, top) flags: pcnn_varcoef_bc_apply - p and q cover the unknowns of varcoef_unknowns, a Neumann edge's nodes
    included, and pq is the weighted sum w p q (varcoef_weights).  None: the all-Dirichlet entry point.
    reaction: c (N,H,W) fp32 on every node -> q = (A + C) p, C = diag(c) on the unknowns (pcnn_varcoef_bc_apply_reaction; with
    neumann = None its mask 0).  None: the calls above, untouched."""
    if rho.dim() != 3:
        raise ValueError('rho must be (N,H,W)')
    N, H, W = rho.shape
    (i0, i1), (j0, j1) = varcoef_unknowns(H, W, neumann if neumann is not None else (False,) * 4)
    _chk_varcoef(rho, 'rho', (N, H, W))
    _chk_varcoef(dx, 'dx', (N,))
    _chk_varcoef(p, 'p', (N, i1 - i0 + 1, j1 - j0 + 1), torch.float64)
    q = torch.empty_like(p)
    pq = torch.empty((N,), dtype=torch.float64, device=p.device)
    if reaction is not None:
        _chk_varcoef(reaction, 'reaction', (N, H, W))
        handle().call('pcnn_varcoef_bc_apply_reaction', c_int(N), c_int(H), c_int(W), c_int(_neumann_mask(neumann) if neumann is not None else 0), _p(rho), _p(dx),
                      _p(p), _p(q), _p(pq), _p(reaction))
    elif neumann is None:
        handle().call('pcnn_varcoef_apply', c_int(N), c_int(H), c_int(W), _p(rho), _p(dx), _p(p), _p(q), _p(pq))
    else:
        handle().call('pcnn_varcoef_bc_apply', c_int(N), c_int(H), c_int(W), c_int(_neumann_mask(neumann)), _p(rho), _p(dx), _p(p), _p(q), _p(pq))
    return q, pq


# columns of the per-sample scalar table of pcnn_varcoef_pcg_* (8 doubles per sample); wb, bb_raw: sum w b and sum w b^2 before the mask-15 projection
VARCOEF_SCALARS = {'bb': 0, 'rr': 1, 'pq': 2, 'rho_min': 5, 'wb': 6, 'bb_raw': 7}
# ... and of the 4 doubles per sample the *_reaction entry points keep behind that table: the weighted means of c and of 1/rho, the minimum of c
VARCOEF_REACTION_SCALARS = {'c_mean': 0, 'inv_rho_mean': 1, 'c_min': 2}


def varcoef_pcg_solve(rho, rhs, left, right, bottom, top, dx, tol=1e-10, max_iterations=500, x0=None, check_every=8, check_start=False, neumann=None,
                      scaled=False, reaction=None):
    """Preconditioned conjugate gradients on the variable-density system (pcnn_varcoef_pcg_setup / _iterate / _finish).  rho, rhs (N,H,W),
    left/right (N,W), bottom/top (N,H), dx (N,): fp32 CUDA tensors; x0: optional (N,H,W) fp64 initial guess (its unknowns are used).
    The device runs check_every iterations per call; the host reads the N convergence flags between calls and nothing else.
    -> soln (N,H,W) fp32 and a dict of host arrays: iterations (the multiple of check_every at which the sample's flag was seen; for a sample that
    did not converge, all that were run), converged, relative_residual = ||r|| / ||b|| of the recurrence, rho_min, compatibility_defect, rhs_shift.
    check_start: also read the flags the setup launch raised for the start itself (||b - A x0|| <= tol ||b||): such a sample reports 0 iterations,
    and no iteration is launched when every sample has one.  The solution's bits are the same either way - a flagged sample is frozen.
    A rho that is not positive everywhere (NaN included) raises ValueError straight after the setup launch.
    neumann = (left, right, bottom, top) flags: the pcnn_varcoef_bc_pcg_* entry points (include/pcnn.h) - a flagged edge's array holds du/dn along
    the outward normal and its nodes are unknowns; norms are those of the W inner product.  None: the all-Dirichlet entry points; four False flags
    run the same problem through the *_bc_* ones and give the same bits.  All four True: the data need not be compatible - setup projects b, and
    compatibility_defect = |sum w b| / sqrt(sum w * sum w b^2) in [0, 1] says how far it was; rhs_shift is the constant (sum w b) / (sum w) the
    projection took from b, i.e. the solution solves the system of rhs + rhs_shift; the solution has zero trapezoidal integral.  Both are 0
    for every other mask.
    scaled: the *_scaled entry points - the preconditioner s o M^-1 (s o r), s = (mean face coefficient)^-1/2, for smooth rho;
    one more workspace field, the same launches per iteration, the same finish.
    reaction: c (N,H,W) fp32 CUDA tensor, read on the unknowns: div((1/rho) grad u) - c u = f through the pcnn_varcoef_bc_*_reaction entry points
    (neumann = None is their mask 0).  A c that is negative, NaN or infinite on an unknown raises ValueError straight after the
    setup launch, as does - with all four edges Neumann - a sample whose c is zero on every unknown (singular: solve it without the keyword).  All
    four True with c > 0 somewhere is nonsingular: no projection, no mean removed, compatibility_defect and rhs_shift are zeros.  Not with scaled.
    None: the calls above, untouched."""
    N, H, W = rho.shape
    if reaction is not None and scaled:
        raise ValueError('the scaled preconditioner has no reaction variant: scaled and reaction exclude each other')
    for name, t, shape in (('rho', rho, (N, H, W)), ('rhs', rhs, (N, H, W)), ('left', left, (N, W)), ('right', right, (N, W)), ('bottom', bottom, (N, H)),
                           ('top', top, (N, H)), ('dx', dx, (N,))):
        _chk_varcoef(t, name, shape)
    if x0 is not None:
        _chk_varcoef(x0, 'x0', (N, H, W), torch.float64)
    if reaction is not None:
        _chk_varcoef(reaction, 'reaction', (N, H, W))
    if not (tol > 0 and max_iterations >= 1 and check_every >= 1):
        raise ValueError('tol must be positive, max_iterations and check_every at least 1')
    dev = rho.device
    lib, h = _lib.load(), handle()
    # the three stages as closures, one set per family of entry points: every call site spelled out (tools/check_ctypes_calls.py reads them)
    if reaction is not None:
        mask = _neumann_mask(neumann) if neumann is not None else 0
        Vih, Vh, lh, ViwT, VwT, lw = _varcoef_bases(H, W, neumann if neumann is not None else (False,) * 4, dev)
        nbytes = int(lib.pcnn_varcoef_bc_pcg_workspace_reaction(c_int(N), c_int(H), c_int(W), c_int(mask)))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        setup = lambda: h.call('pcnn_varcoef_bc_pcg_setup_reaction', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(rhs), _p(left), _p(right), _p(bottom),
                               _p(top), _p(dx), _p(x0), c_double(tol), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal_all),
                               _p(flags), _p(reaction))
        iterate = lambda it: h.call('pcnn_varcoef_bc_pcg_iterate_reaction', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(dx), c_double(tol), c_int(it),
                                    c_int(check_every), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal_all), _p(flags),
                                    _p(reaction))
        finish = lambda: h.call('pcnn_varcoef_bc_pcg_finish_reaction', c_int(N), c_int(H), c_int(W), c_int(mask), _p(ws), _p(left), _p(right), _p(bottom), _p(top),
                                _p(soln))
    elif neumann is None:
        Sh, lh = dst_matrices(H, dev)
        Sw, lw = dst_matrices(W, dev)
        nbytes = int(lib.pcnn_varcoef_pcg_workspace_scaled(c_int(N), c_int(H), c_int(W)) if scaled else lib.pcnn_varcoef_pcg_workspace(c_int(N), c_int(H), c_int(W)))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        setup = lambda: h.call('pcnn_varcoef_pcg_setup', c_int(N), c_int(H), c_int(W), _p(rho), _p(rhs), _p(left), _p(right), _p(bottom), _p(top), _p(dx), _p(x0),
                               c_double(tol), _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
        iterate = lambda it: h.call('pcnn_varcoef_pcg_iterate', c_int(N), c_int(H), c_int(W), _p(rho), _p(dx), c_double(tol), c_int(it), c_int(check_every),
                                    _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
        finish = lambda: h.call('pcnn_varcoef_pcg_finish', c_int(N), c_int(H), c_int(W), _p(ws), _p(left), _p(right), _p(bottom), _p(top), _p(soln))
        if scaled:
            setup = lambda: h.call('pcnn_varcoef_pcg_setup_scaled', c_int(N), c_int(H), c_int(W), _p(rho), _p(rhs), _p(left), _p(right), _p(bottom), _p(top), _p(dx),
                                   _p(x0), c_double(tol), _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
            iterate = lambda it: h.call('pcnn_varcoef_pcg_iterate_scaled', c_int(N), c_int(H), c_int(W), _p(rho), _p(dx), c_double(tol), c_int(it),
                                        c_int(check_every), _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
    else:
        mask = _neumann_mask(neumann)
        Vih, Vh, lh, ViwT, VwT, lw = _varcoef_bases(H, W, neumann, dev)
        nbytes = int(lib.pcnn_varcoef_bc_pcg_workspace_scaled(c_int(N), c_int(H), c_int(W), c_int(mask)) if scaled else
                     lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(mask)))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        setup = lambda: h.call('pcnn_varcoef_bc_pcg_setup', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(rhs), _p(left), _p(right), _p(bottom), _p(top),
                               _p(dx), _p(x0), c_double(tol), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
        iterate = lambda it: h.call('pcnn_varcoef_bc_pcg_iterate', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(dx), c_double(tol), c_int(it),
                                    c_int(check_every), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
        finish = lambda: h.call('pcnn_varcoef_bc_pcg_finish', c_int(N), c_int(H), c_int(W), c_int(mask), _p(ws), _p(left), _p(right), _p(bottom), _p(top),
                                _p(soln))
        if scaled:
            setup = lambda: h.call('pcnn_varcoef_bc_pcg_setup_scaled', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(rhs), _p(left), _p(right), _p(bottom),
                                   _p(top), _p(dx), _p(x0), c_double(tol), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal),
                                   _p(flags))
            iterate = lambda it: h.call('pcnn_varcoef_bc_pcg_iterate_scaled', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(dx), c_double(tol), c_int(it),
                                        c_int(check_every), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
    if reaction is None:
        scal = torch.empty((N, 8), dtype=torch.float64, device=dev)              # (the closures above find scal, flags and soln when they are called)
    else:                                                                        # the N x 8 table, then N x 4 more doubles (include/pcnn.h)
        scal_all = torch.empty((N * 12,), dtype=torch.float64, device=dev)
        scal = scal_all[:N * 8].view(N, 8)
    flags = torch.empty((N,), dtype=torch.int32, device=dev)
    setup()
    if reaction is None:
        rho_min = scal[:, VARCOEF_SCALARS['rho_min']].cpu().numpy()
    else:                                                               # one read for both tables
        s0 = scal_all.cpu().numpy()
        rho_min, extra = s0[:N * 8].reshape(N, 8)[:, VARCOEF_SCALARS['rho_min']], s0[N * 8:].reshape(N, 4)
    if not np.all(rho_min > 0):                                         # the setup kernel's minimum counts a NaN as -inf; nothing more is launched
        raise ValueError('rho must be positive everywhere (minimum per sample: %r)' % (rho_min.tolist(),))
    if reaction is not None:
        c_min, c_mean = extra[:, VARCOEF_REACTION_SCALARS['c_min']], extra[:, VARCOEF_REACTION_SCALARS['c_mean']]
        if not np.all(c_min >= 0):                                      # (a NaN or an infinity counts as -inf there)
            raise ValueError('reaction must be non-negative and finite on every unknown (minimum per sample: %r)' % (c_min.tolist(),))
        if mask == 15 and not np.all(c_mean > 0):
            raise ValueError('all four edges Neumann and a reaction that is zero on every unknown of sample(s) %r: that system is singular - solve such a '
                             'sample without the reaction keyword' % (np.flatnonzero(~(c_mean > 0)).tolist(),))
    iterations = np.zeros(N, dtype=np.int64)
    done = (flags.cpu().numpy() != 0) if check_start else np.zeros(N, dtype=bool)
    it = 0
    while it < max_iterations and not done.all():
        iterate(it)
        it += check_every
        f = flags.cpu().numpy() != 0                                    # the one host read per check_every iterations
        iterations[f & ~done] = it
        done |= f
    iterations[~done] = it
    soln = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    finish()
    s = scal.cpu().numpy()
    bb, rr, wb, raw = (s[:, VARCOEF_SCALARS[k]] for k in ('bb', 'rr', 'wb', 'bb_raw'))
    sum_w = float((H - 1) * (W - 1))                                    # of mask 15, the only mask with wb, raw != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1.0)), 0.0)
        defect = np.where(raw > 0, np.abs(wb) / np.sqrt(sum_w * np.where(raw > 0, raw, 1.0)), 0.0)
    return soln, {'iterations': iterations, 'converged': done, 'relative_residual': rel, 'rho_min': rho_min, 'compatibility_defect': defect,
                  'rhs_shift': wb / sum_w}


def varcoef_density(g, lo, hi):
    """In place: g -> lo + (hi - lo) min(|g|, 1) (pcnn_varcoef_density); g: a smooth fp32 field scaled to max|g| = 1."""
    if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
        raise ValueError('varcoef_density takes a contiguous CUDA float32 tensor')
    handle().call('pcnn_varcoef_density', c_int64(g.numel()), c_float(lo), c_float(hi), _p(g))
    return g


def varcoef_reaction_field(g, lo, hi):
    """varcoef_density's map by the same kernel for a reaction field: 0 <= lo <= hi (pcnn_varcoef_reaction_field)."""
    if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
        raise ValueError('varcoef_reaction_field takes a contiguous CUDA float32 tensor')
    handle().call('pcnn_varcoef_reaction_field', c_int64(g.numel()), c_float(lo), c_float(hi), _p(g))
    return g


def varcoef_density_smooth(g, lo, hi):
    """In place: g[n] -> lo + (hi - lo) (g[n] - min g[n]) / (max g[n] - min g[n]) (pcnn_varcoef_density_smooth); g (N, ...): fp32, any scale."""
    if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous() or g.dim() < 2:
        raise ValueError('varcoef_density_smooth takes a contiguous CUDA float32 tensor with a leading sample axis')
    handle().call('pcnn_varcoef_density_smooth', c_int(g.shape[0]), c_int64(g.numel() // g.shape[0]), c_float(lo), c_float(hi), _p(g))
    return g


def varcoef_series_pair(coef, rho, dx, neumann=(False, False, False, False)):
    """coef (N,ka,kb), rho (N,H,W), dx (N,), `neumann` = (left, right, bottom, top) -> (soln, rhs), each (N,H,W): the series of the edge types'
    eigenfunction families and the discrete right-hand side L_h(rho) soln of the same launch (ops.varcoef_series_pair, pcnn_varcoef_series_pair)."""
    return ops.varcoef_series_pair(coef, rho, dx, _neumann_mask(neumann))


def series_synthesis(coef, H, W, trig, out=None, accumulate=False):
    """coef (N,ka,kb) -> (N,H,W): sum c[A,B] f((A+1)x) f((B+1)y), f = sin (trig=0) / cos (trig=1)."""
    N, ka, kb = coef.shape
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=coef.device)
        accumulate = False
    handle().call('pcnn_series_synthesis', c_int(N), c_int(H), c_int(W), c_int(ka), c_int(kb), _p(coef.contiguous()), c_int(trig),
                  c_int(1 if accumulate else 0), _p(out))
    return out


SERIES_PAIR_TILE = (32, 128)     # rows x columns one block of series_pair_kernel writes (PAIR_ROWS, PAIR_COLS in csrc/dataset.hip)

def series_pair_synthesis(coef, lam_a, lam_b, H, W, basis_a, basis_b):
    """coef (N,ka,kb), lam_a (N,ka), lam_b (N,kb) -> (soln, rhs), each (N,H,W), in one launch: soln = sum c[A,B] phi_A(x) psi_B(y) and
    rhs = sum c[A,B] (lam_a[A] + lam_b[B]) phi_A(x) psi_B(y).  basis 0: sin(A t), 1: cos(A t), 2: sin((A-1/2) t), 3: cos((A-1/2) t)."""
    N, ka, kb = coef.shape
    if tuple(lam_a.shape) != (N, ka) or tuple(lam_b.shape) != (N, kb):
        raise ValueError('lam_a (N,ka) and lam_b (N,kb) must match coef (N,ka,kb): got %r, %r, %r' % (tuple(lam_a.shape), tuple(lam_b.shape), tuple(coef.shape)))
    for t in (coef, lam_a, lam_b):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError('series_pair_synthesis takes CUDA float32 tensors')
    soln = torch.empty((N, H, W), dtype=torch.float32, device=coef.device)
    rhs = torch.empty_like(soln)
    handle().call('pcnn_series_pair_synthesis', c_int(N), c_int(H), c_int(W), c_int(ka), c_int(kb), _p(coef.contiguous()), _p(lam_a.contiguous()),
                  _p(lam_b.contiguous()), c_int(basis_a), c_int(basis_b), _p(soln), _p(rhs))
    return soln, rhs


def separable_sum(U, V, out=None, accumulate=False):
    """U (N,R,H), V (N,R,W) -> (N,H,W)"""
    N, R, H = U.shape
    W = V.shape[2]
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=U.device)
        accumulate = False
    handle().call('pcnn_separable_sum', c_int(N), c_int(H), c_int(W), c_int(R), _p(U.contiguous()), _p(V.contiguous()), c_int(1 if accumulate else 0), _p(out))
    return out


def set_max_magnitude(x, target):
    """In place: x[n] *= target[n]/max|x[n]|; returns the factors."""
    N = x.shape[0]
    f = torch.empty((N,), dtype=torch.float32, device=x.device)
    handle().call('pcnn_set_max_magnitude', c_int(N), c_int64(x.numel() // N), _p(target), _p(x), _p(f))
    return f


def scale_samples(x, s):
    N = x.shape[0]
    handle().call('pcnn_scale_samples', c_int(N), c_int64(x.numel() // N), _p(s), _p(x))
    return x


def max_abs_per_sample(x):
    """max|x[n]| via the loss partial-sum kernel (column 3)."""
    return ops.loss_partials(x, x, None)[:, 3].contiguous()


def resize_legacy_bicubic(x, out_hw):
    """tf.compat.v1.image.resize_images(BICUBIC, align_corners=True) of (N,h,w,C) (dataset/utils/image_resize.py:20)."""
    return ops.resize_fwd(x, out_hw, 'bicubic_legacy')
