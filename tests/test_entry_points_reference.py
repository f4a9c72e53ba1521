"""The NumPy twin of the pipeline-only entry points (tests/entry_points_twin.py), on the very inputs tests/test_gpu_entry_points.py gives the kernels - no GPU
needed.  Per operation: the twin agrees with an independently written form (index loops, index arithmetic, torch autograd or the oracle) to 1e-12 or exactly;
its float32 evaluation stays under the bound the GPU test applies; and a deliberately wrong variant - one indexing or layout slip the kernel could have - misses
that bound, so the inputs are not too symmetric to see it.  A variant is skipped only where its index map IS the right one (a unit axis, a 1 x 1 product,
a sine series on a single point, which is zero whatever the modes): each test states the condition."""
import os

import numpy as np
import pytest
import torch

from oracle import dataset as ods, dbcnn as odb, hpnn as ohpnn, np_ops
from tests import entry_points_twin as T

F = np.float32


def close(a, b):
    """1e-12 relative to the size of the reference (exactly, where the reference is zero)."""
    return T.rel(a, b) <= 1e-12


# ----------------------------------------------------------------------------- 1. fp64 GEMM
def _tiles16_transposed(A):
    """Every 16 x 16 tile of the zero-padded matrices transposed in place: the operand tile read with its row and column lanes exchanged."""
    *lead, M, K = A.shape
    Mp, Kp = -(-M // 16) * 16, -(-K // 16) * 16
    P = np.zeros((*lead, Mp, Kp))
    P[..., :M, :K] = A
    P = P.reshape(*lead, Mp // 16, 16, Kp // 16, 16).swapaxes(-3, -1).reshape(*lead, Mp, Kp)
    return P[..., :M, :K]


def _wrong_row_map(C):
    """The accumulator register `reg` of lane group `lq` stored to row 4 lq + reg of its 16-row group instead of lq + 4 reg."""
    *lead, M, N = C.shape
    Mp = -(-M // 16) * 16
    P = np.zeros((*lead, Mp, N))
    P[..., :M, :] = C
    j = np.arange(16)
    src = j // 4 + 4 * (j % 4)                                   # row 4 lq + reg = j receives what belongs to row lq + 4 reg
    return P.reshape(*lead, Mp // 16, 16, N)[..., src, :].reshape(*lead, Mp, N)[..., :M, :]


@pytest.mark.parametrize('kind', T.GEMM_KINDS)
@pytest.mark.parametrize('form', T.GEMM_FORMS)
@pytest.mark.parametrize('M,N,K', T.GEMM_SHAPES)
def test_gemm_twin_and_its_wrong_variants(M, N, K, form, kind):
    """Skipped variants: a transposed A tile at M = K = 1, a transposed B tile at K = N = 1, the row map at M = 1 (row 0 is row 0 under both maps)."""
    A, B = T.gemm_inputs(M, N, K, form, kind)
    C = T.gemm(A, B)
    loops = sum(A[:, :, k, None] * B[:, k, None, :] for k in range(K))
    assert C.shape == (1 if form == 'single' else 3, M, N)
    assert np.array_equal(C, loops) if kind == 'int' else close(C, loops)
    bound = T.gemm_bound(A, B)
    missed = (lambda Cw: not np.array_equal(Cw, C)) if kind == 'int' else (lambda Cw: bool((np.abs(Cw - C) > bound).any()))
    if kind == 'int':
        assert np.abs(A).max() <= 8 and np.abs(B).max() <= 8 and np.array_equal(A, np.round(A))
    if M > 1 or K > 1:
        assert missed(T.gemm(_tiles16_transposed(A), B))
    if K > 1 or N > 1:
        assert missed(T.gemm(A, _tiles16_transposed(B)))
    if M > 1:
        assert missed(_wrong_row_map(C))


# ----------------------------------------------------------------------------- 2. series synthesis
def _series_cases(ka):
    return T.SERIES_SHAPES + ([T.SERIES_WIDEST] if ka == 16 else [])


@pytest.mark.parametrize('trig', [0, 1])
@pytest.mark.parametrize('ka,kb', T.SERIES_MODES)
def test_series_twin_its_float32_error_and_its_wrong_variants(ka, kb, trig):
    """Skipped variants: all three for a sine series with a unit axis (sin of the single point 0: the field is zero whatever the modes and the grid);
    linspace over n and A for A + 1 at (1, 1), where the only grid point is 0 and every cosine is 1."""
    c = T.series_inputs(ka, kb)
    for H, W in _series_cases(ka):
        ref = T.series(c, H, W, trig)
        orc = np.stack([ods.generate_smooth_function((H, W), **{'cos_coeff' if trig else 'sin_coeff': c[n]}) for n in range(2)])
        assert np.abs(ref - orc).max() <= 1e-12 * max(np.abs(orc).max(), 1.0), (H, W)
        bound = T.bound_of(T.SERIES_TOL, T.SERIES_MEASURED, (ka, kb, trig, H, W))
        e32 = T.rel(T.series(c.astype(F), H, W, trig), ref)
        print('series %dx%d trig %d at %dx%d: float32 %.3g, bound %.3g' % (ka, kb, trig, H, W, e32, bound))
        assert e32 < bound and T.SERIES_MEASURED.get((ka, kb, trig, H, W), 0.0) <= 1.1 * e32, (H, W, e32)     # under the bound, and the table does not overstate it
        if (H, W) in T.SERIES_ACC_SHAPES:
            base = T.series_base(H, W)
            assert np.array_equal(T.series(c, H, W, trig, base), base + ref)
            assert T.rel(T.series(c.astype(F), H, W, trig, base.astype(F)), base + ref) < bound
        if trig == 0 and min(H, W) == 1:
            assert not ref.any()
            continue
        if (H, W) != (1, 1):
            assert T.rel(T._series(c, H, W, trig, over_n=True), ref) > bound, (H, W)
            assert T.rel(T._series(c, H, W, trig, first_mode=0), ref) > bound, (H, W)
        assert T.rel(T._series(c, H, W, trig, swap=True), ref) > bound, (H, W)


# ----------------------------------------------------------------------------- 3. separable sums, scale_samples, set_max_magnitude
@pytest.mark.parametrize('N,H,W,R', [s + (R,) for s in T.SEPSUM_SHAPES for R in T.SEPSUM_RANKS] + [T.BIG_FIELD + (T.BIG_RANK,)])
def test_separable_sum_twin_and_its_float32_error(N, H, W, R):
    U, V, base = T.sepsum_inputs(N, H, W, R)
    ref = T.separable_sum(U, V)
    assert close(ref, sum(U[:, r, :, None] * V[:, r, None, :] for r in range(R)))
    assert np.array_equal(T.separable_sum(U, V, base), base + ref)
    e32 = max(T.rel(T.separable_sum(U.astype(F), V.astype(F)), ref), T.rel(T.separable_sum(U.astype(F), V.astype(F), base.astype(F)), base + ref))
    print('separable_sum %r R %d: float32 %.3g' % ((N, H, W), R, e32))
    assert e32 < T.SEPSUM_TOL / 4
    if R > 1:                                                    # U[n, r] read as U[r, n] of the flat array (R = 1: the same element)
        assert T.rel(T.separable_sum(U.reshape(R, N, H).transpose(1, 0, 2), V), ref) > T.SEPSUM_TOL


@pytest.mark.parametrize('shape', T.SEPSUM_SHAPES + [T.BIG_FIELD])
def test_sample_scalings_twin(shape):
    x, s = T.field_inputs(shape)
    y = T.scale_samples(x, s)
    assert all(np.array_equal(y[n], x[n] * s[n]) for n in range(shape[0]))
    assert T.rel(T.scale_samples(x.astype(F), s.astype(F)), y) < T.TOL
    assert T.rel(T.scale_samples(x, s[::-1]), y) > T.TOL         # s[N - 1 - n]
    z, fac = T.set_max_magnitude(x, np.abs(s))
    assert close(z, np.stack([np_ops.set_max_magnitude_in_batch(x[n:n + 1, None], abs(s[n]))[0, 0] for n in range(shape[0])]))
    assert np.allclose(np.abs(z).reshape(shape[0], -1).max(1), np.abs(s), rtol=1e-14)


# ----------------------------------------------------------------------------- 4. sub-sampling
def _sub_bwd_by_index(dy, H, W, s, swap=False):
    """The kernel's own form: every fine element looks its coarse one up at (n Ho + yy / s) Wo + xx / s.  swap: Wo and Ho exchanged in that index."""
    N, Ho, Wo, C = dy.shape
    n, yy, xx = np.arange(N)[:, None, None], np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    A, B = (Wo, Ho) if swap else (Ho, Wo)
    at = ((n * A + yy // s) * B + xx // s) % (N * Ho * Wo)
    return np.where(((yy % s == 0) & (xx % s == 0))[..., None], dy.reshape(-1, C)[at], 0.0)


@pytest.mark.parametrize('s', T.SUB_STRIDES)
def test_subsample_twin_and_its_wrong_variants(s):
    """Skipped variant: Ho / Wo exchanged where Ho = Wo or Ho = 1 (the same flat index)."""
    cases = [(H, W, C, s, 2) for H, W in T.SUB_GRIDS for C in T.SUB_CHANNELS] + ([T.SUB_BIG[1:] + (s, T.SUB_BIG[0])] if s == T.SUB_BIG_STRIDE else [])
    for H, W, C, _, N in cases:
        x, dy = T.sub_inputs(H, W, C, s, N)
        Ho, Wo = -(-H // s), -(-W // s)
        y = T.subsample(x, s)
        assert y.shape == dy.shape == (N, Ho, Wo, C)
        assert np.array_equal(y, x[:, np.arange(Ho) * s][:, :, np.arange(Wo) * s])
        if x.size < 10000:
            assert all(y[n, i, j, c] == x[n, i * s, j * s, c] for n in range(N) for i in range(Ho) for j in range(Wo) for c in range(C))
        dx = T.subsample_bwd(dy, (H, W), s)
        assert np.array_equal(dx, _sub_bwd_by_index(dy, H, W, s))
        assert np.count_nonzero(dx) == dy.size
        if x.size < 10000:
            assert (x * dx).sum() == (y * dy).sum()                                         # the adjoint identity, exact on these integers
        off = x[:, 1::s, 1::s, :]                                                           # the lattice offset by one
        assert off.shape != y.shape or not np.array_equal(off, y)
        assert x[:, ::s + 1, ::s + 1, :].shape != y.shape or not np.array_equal(x[:, ::s + 1, ::s + 1, :], y) or (Ho == 1 and Wo == 1)
        if Ho != Wo and Ho > 1:
            assert not np.array_equal(_sub_bwd_by_index(dy, H, W, s, swap=True), dx), (H, W, C)


# ----------------------------------------------------------------------------- 5. input assembly
def _cos_wrong(n, over_n=False, sin=False):
    t = np.arange(n) / n if over_n else T.linspace01(n)
    return (np.sin if sin else np.cos)(np.pi * t)


@pytest.mark.parametrize('n', sorted({n for hw in T.ASM_GRIDS for n in hw} | set(T.DBC_LENGTHS) | set(T.ASM_BIG[1:]) | {n for s in T.DBC_EXPAND_SHAPES for n in s[1:3]}))
def test_cosine_channel_its_float32_error_and_its_wrong_variants(n):
    """Skipped variant: linspace over n at n = 1, where both are [0]."""
    ref = T.cos_channel(n)
    assert close(ref, [np.cos(np.pi * i / (n - 1)) if n > 1 else 1.0 for i in range(n)])
    e32 = np.abs(T.cos_channel(n, F).astype(np.float64) - ref).max()
    print('cos channel n = %d: float32 max-abs %.3g' % (n, e32))
    assert T.cos_channel(n, F).dtype == F and e32 < T.COS_TOL / 4
    if n == 1:
        assert ref.tolist() == [1.0] and T.cos_channel(1, F).tolist() == [1.0]
    else:
        assert np.abs(_cos_wrong(n, over_n=True) - ref).max() > T.COS_TOL
    assert np.abs(_cos_wrong(n, sin=True) - ref).max() > T.COS_TOL


@pytest.mark.parametrize('H,W', T.ASM_GRIDS + [T.ASM_BIG[1:]])
def test_assembly_twins(H, W):
    N = 3
    stack = T.asm_inputs(N, H, W)
    pos = ohpnn.position_embeddings(np_ops, N, H, W)                                        # (N, 2, H, W): along y, along x
    for use_pos in (True, False):
        a = T.assemble_input(stack[:, 0], use_pos)
        d = T.assemble_density_input(stack, use_pos)
        assert a.shape == (N, H, W, 3 if use_pos else 1) and d.shape == (N, H, W, 4 if use_pos else 2)
        assert np.array_equal(a[..., 0], stack[:, 0]) and np.array_equal(d[..., :2], stack.transpose(0, 2, 3, 1))
        if use_pos:
            assert close(a[..., 1:], pos.transpose(0, 2, 3, 1)) and close(d[..., 2:], pos.transpose(0, 2, 3, 1))
            if H != W:                                                                      # y and x exchanged
                assert np.abs(a[..., 1] - pos[:, 1]).max() > T.COS_TOL
    assert T.assemble_input(stack[:, 0].astype(F)).dtype == F


@pytest.mark.parametrize('L', T.DBC_LENGTHS)
def test_dbc_assembly_twin(L):
    bc = T.bc_inputs(3, L)
    out = T.dbc_assemble_input(bc)
    assert out.shape == (3, 1, L, 3)
    assert np.array_equal(out[:, 0, :, 0], bc) and (out[..., 1] == 1.0).all()
    assert close(out[:, 0, :, 2], odb.position_embeddings(3, 1, L)[:, 1, 0])


# ----------------------------------------------------------------------------- 6. first row
@pytest.mark.parametrize('N,X,L', T.FIRST_ROW_SHAPES)
def test_set_first_row_twin(N, X, L):
    y, bc = T.field_inputs((N, X, L))[0], T.bc_inputs(N, L)
    for b in (bc, None):
        out = T.set_first_row(y, b)
        assert all(out[n, x, c] == ((b[n, c] if b is not None else 0.0) if x == 0 else y[n, x, c]) for n in range(N) for x in range(X) for c in range(L))
    if X > 1:
        wrong = y.copy()
        wrong.reshape(N * X, L)[:N] = bc                                                    # the sample stride X L forgotten
        assert not np.array_equal(wrong, T.set_first_row(y, bc))


# ----------------------------------------------------------------------------- 7. flip / rotate
@pytest.mark.parametrize('shape', T.FLIP_SHAPES + [T.FLIP_BIG])
def test_flip_rotate_twin_and_exchanged_flips(shape):
    """The eight index maps against the kernel's header formula out[n, a, b] = in[n, src(a, b)]; flip_y and flip_x exchanged under transpose must differ
    whenever exactly one of them is set."""
    x, alpha, base_t, base = T.flip_inputs(shape)
    N, H, W = shape
    for t, fy, fx in (T.FLIP_COMBOS if shape != T.FLIP_BIG else [T.FLIP_BIG_COMBO]):
        out = T.flip_rotate(x, t, fy, fx)
        Ho, Wo = (W, H) if t else (H, W)
        a, b = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
        a2, b2 = (Ho - 1 - a if fy else a), (Wo - 1 - b if fx else b)
        sy, sx = (b2, a2) if t else (a2, b2)
        assert out.shape == (N, Ho, Wo) and np.array_equal(out, x[:, sy, sx])
        if x.size < 1000:
            rc = {(False, False, False): (0, ()), (False, True, False): (0, (2,)), (False, False, True): (0, (3,)), (False, True, True): (2, ()),
                  (True, False, False): (1, (2,)), (True, True, False): (1, ()), (True, False, True): (3, ()), (True, True, True): (3, (2,))}[(t, fy, fx)]
            assert np.array_equal(out, odb.flip_and_rotate(np_ops, x[:, None], rotation_count=rc[0], flip_axes=rc[1])[:, 0])
        b0 = base_t if t else base
        acc = T.flip_rotate(x, t, fy, fx, alpha, b0)
        assert all(np.array_equal(acc[n], b0[n] + alpha[n] * out[n]) for n in range(N))
        assert T.rel(T.flip_rotate(x.astype(F), t, fy, fx, alpha.astype(F), b0.astype(F)), acc) < T.TOL
        if t and fy != fx:
            assert not np.array_equal(T.flip_rotate(x, t, fx, fy), out)


# ----------------------------------------------------------------------------- 8. boundary expansion
@pytest.mark.parametrize('N,X,L,M', T.DBC_EXPAND_SHAPES)
def test_dbc_expand_twin_its_adjoint_and_its_float32_error(N, X, L, M):
    """Forward against torch's einsum('bmy,mx,bm->bmxy') and the oracle's embedding channels, backward against its autograd.  Skipped variant: d read as
    d[m, n] of the flat array at M = 1, where it is the same element."""
    f, sh, d, dout = T.dbc_inputs(N, X, L, M)
    out = T.dbc_expand(f, sh, d)
    ft, dt = torch.tensor(f[:, 0].transpose(0, 2, 1).copy(), requires_grad=True), torch.tensor(d, requires_grad=True)      # (N, M, L)
    prod = torch.einsum('bmy,mx,bm->bmxy', ft, torch.tensor(sh), dt)
    assert out.shape == (N, X, L, M + 2) and close(out[..., :M], prod.detach().numpy().transpose(0, 2, 3, 1))
    assert close(out[..., M:], odb.position_embeddings(N, X, L).transpose(0, 2, 3, 1))
    if X == 1:
        assert (out[..., M] == 1.0).all()
    if L == 1:
        assert (out[..., M + 1] == 1.0).all()
    (prod * torch.tensor(dout[..., :M].transpose(0, 3, 1, 2).copy())).sum().backward()
    df, dd = T.dbc_expand_bwd(dout, f, sh, d)
    assert df.shape == (N, 1, L, M) and close(df[:, 0], ft.grad.numpy().transpose(0, 2, 1)) and close(dd, dt.grad.numpy())
    c = lambda *a: [v.astype(F) for v in a]
    o32, (df32, dd32) = T.dbc_expand(*c(f, sh, d)), T.dbc_expand_bwd(*c(dout, f, sh, d))
    e = (T.rel(o32[..., :M], out[..., :M]), T.rel(df32, df), T.rel(dd32, dd), np.abs(o32[..., M:].astype(np.float64) - out[..., M:]).max())
    print('dbc_expand %r: float32 product %.3g, df %.3g, dd %.3g, embedding max-abs %.3g' % (((N, X, L, M),) + e))
    assert e[0] < T.DBC_FWD_TOL / 4 and e[1] < T.DBC_BWD_TOL / 4 and e[2] < T.DBC_BWD_TOL / 4 and e[3] < T.COS_TOL / 4
    if M > 1:
        dw = d.reshape(M, N).T
        assert T.rel(T.dbc_expand(f, sh, dw)[..., :M], out[..., :M]) > T.DBC_FWD_TOL
        assert T.rel(T.dbc_expand_bwd(dout, f, sh, dw)[0], df) > T.DBC_BWD_TOL
    if X > 1:                                                    # sh[m, x] read as sh[x, m] of the flat array
        assert T.rel(T.dbc_expand(f, sh.reshape(X, M).T, d)[..., :M], out[..., :M]) > T.DBC_FWD_TOL or M == 1


# ----------------------------------------------------------------------------- 9. per-channel and per-sample scaling
@pytest.mark.parametrize('shape', [(3,) + T.SCALE_GRID + (C,) for C in T.SCALE_CHANNELS] + [T.SCALE_BIG])
def test_scaling_twins(shape):
    x, s, g = T.scale_inputs(shape)
    y, z = T.channel_scale(x, s), T.sample_scale(x, g)
    assert np.array_equal(y, np.einsum('nhwc,nc->nhwc', x, s)) and all(np.array_equal(z[n], x[n] * (1 + g[n])) for n in range(shape[0]))
    assert T.rel(T.channel_scale(x.astype(F), s.astype(F)), y) < T.TOL and T.rel(T.sample_scale(x.astype(F), g.astype(F)), z) < T.TOL
    if shape[3] > 1:                                             # s[n, c] read as s[c, n] of the flat array
        assert T.rel(T.channel_scale(x, s.reshape(shape[3], shape[0]).T), y) > T.TOL
    assert T.rel(x * g[:, None, None, None], z) > T.TOL          # the 1 + forgotten


# ----------------------------------------------------------------------------- the cross-reference that motivated these tests
WRAPPERS = ['subsample', 'subsample_bwd', 'assemble_density_input', 'dbc_assemble_input', 'set_first_row', 'scale_samples', 'assemble_input', 'channel_scale_fwd',
            'sample_scale_fwd', 'separable_sum', 'dbc_expand_fwd', 'dbc_expand_bwd', 'series_synthesis', 'flip_rotate']


def test_every_listed_entry_point_is_named_in_the_gpu_test():
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_entry_points.py')) as fh:
        src = fh.read()
    assert "'pcnn_batched_gemm_f64'" in src
    missing = [w for w in WRAPPERS if not re.search(r'\b(ops|K)\.%s\(' % w, src)]
    assert not missing, missing
