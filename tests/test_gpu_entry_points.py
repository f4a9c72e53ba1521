"""Direct parity tests of the entry points that were only reached through a model forward pass, a training step or a Poisson solve: the fp64 matrix-core GEMM,
series synthesis, separable sums, sub-sampling and its adjoint, the input assemblies, the first-row overwrite, flip / rotate, the boundary expansion and the
forward scalings - each against the float64 formula of tests/entry_points_twin.py at small awkward shapes: tile tails, unit axes, leading dimensions larger than
the row, accumulate modes, and one size past the capped grid of each element-wise kernel.

The cases, the inputs and the bounds come from the twin module; tests/test_entry_points_reference.py checks on the CPU that the twin is right on these inputs,
that its float32 evaluation stays under every bound used here and that a kernel with one indexing slip would miss them.

An output the test allocates is filled with NaN before a kernel overwrites it and with a known base before a kernel accumulates into it.  A tensor whose leading
dimension exceeds its row is a view into a wider buffer of SENTINEL, and the columns outside the view must come back bit for bit."""
from ctypes import c_int, c_int64

import numpy as np
import pytest
import torch

from tests import entry_points_twin as T

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
GRID_CAP = T.GRID_CAP           # threads of the capped grid of csrc/pointwise.hip; csrc/dataset.hip and csrc/dbcnn.hip cap at T.DATASET_CAP
rel = T.rel


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device='cuda')


def framed(shape, off=1, extra=3, fill=float('nan'), dtype=torch.float32):
    """(buffer, view): the view has `shape` and sits at columns off .. off + shape[-1] of a buffer that is `extra` columns wider and holds SENTINEL."""
    buf = torch.full(tuple(shape[:-1]) + (shape[-1] + extra,), SENTINEL, dtype=dtype, device='cuda')
    view = buf[..., off:off + shape[-1]]
    if isinstance(fill, float):
        view.fill_(fill)
    else:
        view.copy_(dev(fill, dtype))
    return buf, view


def frame_intact(buf, view, off=1):
    """The columns of buf outside the view still hold SENTINEL."""
    c = view.shape[-1]
    return bool((buf[..., :off] == SENTINEL).all()) and bool((buf[..., off + c:] == SENTINEL).all())


# ----------------------------------------------------------------------------- 1. fp64 batched GEMM on the f64 matrix cores
def run_gemm(A, B, form, pad=0):
    """C = A B through pcnn_batched_gemm_f64 with every leading dimension `pad` past its row; returns C and whether the padding columns kept SENTINEL."""
    from poisson_cnn_amd import ops
    batch, (M, K), N = (1 if form == 'single' else 3), A.shape[1:], B.shape[2]
    Ab, Av = framed(A.shape, 0, pad, A, torch.float64)
    Bb, Bv = framed(B.shape, 0, pad, B, torch.float64)
    Cb, Cv = framed((batch, M, N), 0, pad, dtype=torch.float64)
    sA, sB = (0 if form == 'shared_a' else M * (K + pad)), (0 if form == 'shared_b' else K * (N + pad))
    ops.handle().call('pcnn_batched_gemm_f64', c_int(batch), c_int(M), c_int(N), c_int(K), ops._p(Ab), c_int64(sA), c_int(K + pad), ops._p(Bb), c_int64(sB),
                      c_int(N + pad), ops._p(Cb), c_int64(M * (N + pad)), c_int(N + pad))
    return Cv.cpu().numpy(), all(frame_intact(b, v, 0) for b, v in ((Ab, Av), (Bb, Bv), (Cb, Cv)))


def check_gemm(M, N, K, form, kind, pad=0):
    A, B = T.gemm_inputs(M, N, K, form, kind)
    ref = T.gemm(A, B)
    C, intact = run_gemm(A, B, form, pad)
    assert intact and not np.isnan(C).any()
    if kind == 'int':                                            # exact in any summation order: the lane maps and the tile tails
        assert np.array_equal(C, ref), np.argwhere(C != ref)[:8]
    else:
        excess = np.abs(C - ref) / T.gemm_bound(A, B)
        print('gemm %r %s: max |C - ref| / bound = %.3g' % ((M, N, K), form, excess.max()))
        assert (excess <= 1.0).all()


@pytest.mark.parametrize('kind', T.GEMM_KINDS)
@pytest.mark.parametrize('form', T.GEMM_FORMS)
@pytest.mark.parametrize('M,N,K', T.GEMM_SHAPES)
def test_gemm_f64_tile_tails_and_batch_strides(M, N, K, form, kind):
    """One element, one MFMA, one full 64 x 64 x 16 tile, tails in every dimension, several tiles per axis; batch 1, and batch 3 with A or B shared
    (stride 0), the two forms pcnn_two_sided_gemm_f64 uses."""
    check_gemm(M, N, K, form, kind)


@pytest.mark.parametrize('kind', T.GEMM_KINDS)
@pytest.mark.parametrize('form', ['shared_a', 'shared_b'])
def test_gemm_f64_leading_dimensions_past_the_row(form, kind):
    """lda = K + 3, ldb = N + 3, ldc = N + 3: the three padding columns of every matrix keep their sentinel."""
    check_gemm(*T.GEMM_PADDED, form, kind, pad=3)


def test_gemm_f64_refusals():
    from poisson_cnn_amd import ops
    a = torch.ones(4, dtype=torch.float64, device='cuda')
    c = nans((4,), torch.float64)
    for batch, K in ((65536, 1), (1, 0)):
        with pytest.raises(RuntimeError, match='pcnn_batched_gemm_f64'):
            ops.handle().call('pcnn_batched_gemm_f64', c_int(batch), c_int(1), c_int(1), c_int(K), ops._p(a), c_int64(0), c_int(1), ops._p(a), c_int64(0), c_int(1),
                              ops._p(c), c_int64(0), c_int(1))
    assert bool(torch.isnan(c).all())


# ----------------------------------------------------------------------------- 2. series synthesis
@pytest.mark.parametrize('trig', [0, 1])
@pytest.mark.parametrize('ka,kb', T.SERIES_MODES)
def test_series_synthesis_mode_counts_row_tiles_and_widths(ka, kb, trig):
    """1 and 16 modes per axis and the two mixed counts; H = 1, 15 / 16 / 17 around one 16-row tile, 33 (a third tile); W = 1, 255 / 256 / 257 around one trip of
    the 256 threads; with ka = 16 the widest row the launcher accepts (W = 1008: 64 KiB of LDS); accumulate onto a base."""
    from poisson_cnn_amd.dataset import _kernels as K
    c = T.series_inputs(ka, kb)
    cd = dev(c)
    for H, W in T.SERIES_SHAPES + ([T.SERIES_WIDEST] if ka == 16 else []):
        bound = T.bound_of(T.SERIES_TOL, T.SERIES_MEASURED, (ka, kb, trig, H, W))
        out = nans((2, H, W))
        assert K.series_synthesis(cd, H, W, trig, out=out) is out
        e = rel(host(out), T.series(c, H, W, trig))
        print('series %dx%d trig %d at %dx%d: %.3g (bound %.3g)' % (ka, kb, trig, H, W, e, bound))
        assert e < bound, (H, W, e, bound)
        if (H, W) in T.SERIES_ACC_SHAPES:
            base = T.series_base(H, W)
            acc = K.series_synthesis(cd, H, W, trig, out=dev(base), accumulate=True)
            e = rel(host(acc), T.series(c, H, W, trig, base))
            print('    accumulated: %.3g' % e)
            assert e < bound, (H, W, e, bound)
            assert torch.equal(K.series_synthesis(cd, H, W, trig), out)          # the wrapper's own output tensor


def test_series_synthesis_refusals_leave_the_output_alone():
    """W = 1009 at 16 modes needs 64 KiB + 64 B of LDS; 17 modes on either axis exceed the kernel's register table."""
    from poisson_cnn_amd.dataset import _kernels as K
    for (ka, kb), (H, W) in (((16, 16), (17, 1009)), ((3, 17), (5, 9)), ((17, 3), (5, 9))):
        out = dev(T.series_base(H, W))
        before = out.clone()
        with pytest.raises(RuntimeError, match='pcnn_series_synthesis'):
            K.series_synthesis(dev(np.ones((2, ka, kb))), H, W, 1, out=out, accumulate=True)
        assert torch.equal(out, before)


# ----------------------------------------------------------------------------- 3. separable sums, per-sample scaling, max-magnitude normalisation
@pytest.mark.parametrize('N,H,W,R', [s + (R,) for s in T.SEPSUM_SHAPES for R in T.SEPSUM_RANKS] + [T.BIG_FIELD + (T.BIG_RANK,)])
def test_separable_sum_ranks_a_unit_axis_and_the_grid_cap(N, H, W, R):
    """R = 1, 2, 7; H = 1; overwrite and accumulate; 2 x 1100 x 2000 elements are past the 16384 x 256 threads of the capped grid."""
    from poisson_cnn_amd.dataset import _kernels as K
    U, V, base = T.sepsum_inputs(N, H, W, R)
    ref = T.separable_sum(U, V)
    out = nans((N, H, W))
    K.separable_sum(dev(U), dev(V), out=out)
    e = rel(host(out), ref)
    acc = K.separable_sum(dev(U), dev(V), out=dev(base), accumulate=True)
    ea = rel(host(acc), T.separable_sum(U, V, base))
    print('separable_sum %r R %d: %.3g, accumulated %.3g' % ((N, H, W), R, e, ea))
    assert e < T.SEPSUM_TOL and ea < T.SEPSUM_TOL
    assert rel(host(out)[-1, -1, -300:], ref[-1, -1, -300:]) < T.SEPSUM_TOL and torch.equal(K.separable_sum(dev(U), dev(V)), out)


@pytest.mark.parametrize('shape', T.SEPSUM_SHAPES + [T.BIG_FIELD])
def test_scale_samples_and_set_max_magnitude_in_place(shape):
    from poisson_cnn_amd.dataset import _kernels as K
    x, s = T.field_inputs(shape)
    xd = dev(x)
    assert K.scale_samples(xd, dev(s)) is xd
    ref = T.scale_samples(x, s)
    assert rel(host(xd), ref) < T.TOL and rel(host(xd)[-1].ravel()[-300:], ref[-1].ravel()[-300:]) < T.TOL
    xd = dev(x)
    fac = K.set_max_magnitude(xd, dev(np.abs(s)))
    rz, rf = T.set_max_magnitude(x, np.abs(s))
    assert rel(host(xd), rz) < 1e-6 and np.allclose(host(fac), rf, rtol=1e-5)          # the bounds of tests/test_gpu_stride_edges.py


# ----------------------------------------------------------------------------- 4. strided sub-sampling and its adjoint
def _sub_check(H, W, C, s, N=2):
    from poisson_cnn_amd import ops
    x, dy = T.sub_inputs(H, W, C, s, N)
    y, dx = T.subsample(x, s), T.subsample_bwd(dy, (H, W), s)
    lattice = np.zeros((H, W), bool)
    lattice[::s, ::s] = True
    for sliced in (False, True):
        xd, dyd = dev(x), dev(dy)
        if sliced:                                               # the input is channels 2 .. 2 + C of a tensor 4 channels wider
            xd, dyd = framed(x.shape, 2, 4, x)[1], framed(dy.shape, 2, 4, dy)[1]
            assert ops._ld(xd) == C + 4
        got = ops.subsample(xd, s)
        assert tuple(got.shape) == y.shape and np.array_equal(host(got), y), (H, W, C, s, sliced)
        back = host(ops.subsample_bwd(dyd, (H, W), s))
        assert np.array_equal(back, dx), (H, W, C, s, sliced)
        assert not back[:, ~lattice].any() and np.array_equal(back[:, lattice].reshape(dy.shape), dy)       # exact zeros off the lattice


@pytest.mark.parametrize('s', T.SUB_STRIDES)
def test_subsample_and_its_adjoint_are_exact_copies(s):
    """Strides 1 - 4 on 21 x 26 (no multiple of any stride but 1), 1 x 1, 5 x 1, 4 x 9 with 1, 5 and 8 channels, the input contiguous and a channel slice."""
    for H, W in T.SUB_GRIDS:
        for C in T.SUB_CHANNELS:
            _sub_check(H, W, C, s)


@pytest.mark.parametrize('s', T.SUB_STRIDES)
def test_subsample_writes_into_a_channel_slice(s):
    """ldy = C + 3 in both directions (the wrappers allocate a dense output, so this goes through the handle): the frame keeps its sentinel."""
    from poisson_cnn_amd import ops
    H, W, C = 21, 26, 5
    x, dy = T.sub_inputs(H, W, C, s)
    for adjoint, src, ref in ((0, x, T.subsample(x, s)), (1, dy, T.subsample_bwd(dy, (H, W), s))):
        buf, view = framed(ref.shape)
        sd = framed(src.shape, 2, 4, src)[1]
        ops.handle().call('pcnn_subsample', c_int(2), c_int(H), c_int(W), c_int(C), c_int(s), ops._p(sd), c_int(ops._ld(sd)), ops._p(view), c_int(ops._ld(view)),
                          c_int(adjoint))
        assert np.array_equal(host(view), ref) and frame_intact(buf, view)


def test_subsample_above_the_grid_cap():
    """2 x 1030 x 1024 coarse and 2 x 2060 x 2047 fine elements: both directions take a second trip of the grid-stride loop."""
    N, H, W, C = T.SUB_BIG
    assert N * -(-H // T.SUB_BIG_STRIDE) * -(-W // T.SUB_BIG_STRIDE) * C > GRID_CAP
    _sub_check(H, W, C, T.SUB_BIG_STRIDE, N)


# ----------------------------------------------------------------------------- 5. input assembly
def _check_pos(got, H, W, first):
    """Channels first, first + 1 of an NHWC tensor against cos(pi y / (H - 1)) and cos(pi x / (W - 1)); a unit axis gives exactly cos(0) = 1."""
    for ch, n, shape in ((first, H, (1, H, 1)), (first + 1, W, (1, 1, W))):
        e = np.abs(got[..., ch] - T.cos_channel(n).reshape(shape)).max()
        print('    cosine channel %d over %d points: max-abs %.3g' % (ch, n, e))
        assert e <= T.COS_TOL
        assert n > 1 or (got[..., ch] == 1.0).all()


@pytest.mark.parametrize('H,W', T.ASM_GRIDS + [T.ASM_BIG[1:]])
def test_assemble_input_and_assemble_density_input(H, W):
    """33 x 47, a unit axis on either side, both, 2 x 2 (linspace = [0, 1]) and 840 x 841 (past the grid cap of pcnn_assemble_input)."""
    from poisson_cnn_amd import ops
    N = 3
    stack = T.asm_inputs(N, H, W)
    sd = dev(stack)
    for use_pos in (True, False):
        a = host(ops.assemble_input(sd[:, 0].contiguous(), use_pos))
        d = host(ops.assemble_density_input(sd, use_pos))
        assert a.shape == (N, H, W, 3 if use_pos else 1) and d.shape == (N, H, W, 4 if use_pos else 2)
        assert np.array_equal(a[..., 0], stack[:, 0]) and np.array_equal(d[..., :2], stack.transpose(0, 2, 3, 1))
        assert np.array_equal(a[0, -1, -1, 0], stack[0, 0, -1, -1]) and np.array_equal(a[-1, -1, -1, 0], stack[-1, 0, -1, -1])
        if use_pos:
            _check_pos(a, H, W, 1)
            _check_pos(d, H, W, 2)


@pytest.mark.parametrize('use_pos', [True, False])
def test_assembly_writes_into_a_channel_slice(use_pos):
    """ldo = C + 3 for the three assembly kernels (the wrappers allocate a dense output, so this goes through the handle)."""
    from poisson_cnn_amd import ops
    N, H, W = 3, 33, 47
    stack = T.asm_inputs(N, H, W)
    sd = dev(stack)
    rhs = sd[:, 0].contiguous()
    for name, C, args, ref in (('pcnn_assemble_input', 3 if use_pos else 1, (ops._p(rhs),), T.assemble_input(stack[:, 0], use_pos)),
                               ('pcnn_assemble_density_input', 4 if use_pos else 2, (ops._p(sd),), T.assemble_density_input(stack, use_pos))):
        buf, view = framed((N, H, W, C))
        ops.handle().call(name, c_int(N), c_int(H), c_int(W), *args, c_int(int(use_pos)), ops._p(view), c_int(ops._ld(view)))
        got = host(view)
        k = C - 2 if use_pos else C
        assert np.array_equal(got[..., :k], ref[..., :k]) and np.abs(got - ref).max() <= T.COS_TOL and frame_intact(buf, view)
    bc = T.bc_inputs(N, 61)
    buf, view = framed((N, 1, 61, 3))
    ops.handle().call('pcnn_dbc_assemble_input', c_int(N), c_int(61), ops._p(dev(bc)), ops._p(view), c_int(ops._ld(view)))
    got, ref = host(view), T.dbc_assemble_input(bc)
    assert np.array_equal(got[..., :2], ref[..., :2]) and np.abs(got - ref).max() <= T.COS_TOL and frame_intact(buf, view)


def test_assemble_density_input_refuses_what_it_cannot_read():
    from poisson_cnn_amd import ops
    stack = dev(T.asm_inputs(3, 7, 1))
    wide = dev(T.asm_inputs(3, 33, 47))
    for bad in (wide[:, :, :, ::2], wide.transpose(2, 3), torch.cat([stack, stack[:, :1]], 1), stack.double()):
        with pytest.raises(ValueError, match='assemble_density_input'):
            ops.assemble_density_input(bad)


@pytest.mark.parametrize('L', T.DBC_LENGTHS)
def test_dbc_assemble_input(L):
    from poisson_cnn_amd import ops
    bc = T.bc_inputs(3, L)
    got = host(ops.dbc_assemble_input(dev(bc)))
    assert got.shape == (3, 1, L, 3) and np.array_equal(got[:, 0, :, 0], bc) and (got[..., 1] == 1.0).all()
    e = np.abs(got[:, 0, :, 2] - T.cos_channel(L)).max()
    print('dbc_assemble_input L = %d: cosine channel max-abs %.3g' % (L, e))
    assert e <= T.COS_TOL and (L > 1 or (got[..., 2] == 1.0).all())


# ----------------------------------------------------------------------------- 6. first-row overwrite
@pytest.mark.parametrize('N,X,L', T.FIRST_ROW_SHAPES)
def test_set_first_row_touches_row_zero_only(N, X, L):
    from poisson_cnn_amd import ops
    y, bc = T.field_inputs((N, X, L))[0], T.bc_inputs(N, L)
    for b in (bc, None):
        yd = dev(y)
        before = yd.clone()
        assert ops.set_first_row(yd, dev(b) if b is not None else None) is yd
        assert np.array_equal(host(yd), T.set_first_row(y, b))
        assert torch.equal(yd[:, 1:], before[:, 1:])             # bit for bit


# ----------------------------------------------------------------------------- 7. flip / rotate
@pytest.mark.parametrize('transpose,flip_y,flip_x', T.FLIP_COMBOS)
@pytest.mark.parametrize('shape', T.FLIP_SHAPES)
def test_flip_rotate_index_maps_alpha_and_accumulate(shape, transpose, flip_y, flip_x):
    from poisson_cnn_amd import ops
    x, alpha, base_t, base = T.flip_inputs(shape)
    b0 = base_t if transpose else base
    xd = dev(x)
    plain = T.flip_rotate(x, transpose, flip_y, flip_x)
    got = ops.flip_rotate(xd, transpose, flip_y, flip_x)
    assert tuple(got.shape) == plain.shape and np.array_equal(host(got), plain)
    out = nans(plain.shape)
    ops.flip_rotate(xd, transpose, flip_y, flip_x, out=out)
    assert np.array_equal(host(out), plain)
    out = nans(plain.shape)
    ops.flip_rotate(xd, transpose, flip_y, flip_x, alpha=dev(alpha), out=out)
    assert rel(host(out), T.flip_rotate(x, transpose, flip_y, flip_x, alpha)) < T.TOL
    acc = ops.flip_rotate(xd, transpose, flip_y, flip_x, alpha=dev(alpha), out=dev(b0), accumulate=True)
    assert rel(host(acc), T.flip_rotate(x, transpose, flip_y, flip_x, alpha, b0)) < T.TOL       # (the multiply and the add may fuse: not bit-exact)
    acc = ops.flip_rotate(xd, transpose, flip_y, flip_x, out=dev(b0), accumulate=True)
    assert np.array_equal(host(acc), b0 + plain) or rel(host(acc), b0 + plain) < T.TOL


def test_flip_rotate_above_the_grid_cap():
    from poisson_cnn_amd import ops
    x = T.flip_inputs(T.FLIP_BIG)[0]
    assert x.size > T.DATASET_CAP
    ref = T.flip_rotate(x, *T.FLIP_BIG_COMBO)
    assert np.array_equal(host(ops.flip_rotate(dev(x), *T.FLIP_BIG_COMBO)), ref)


# ----------------------------------------------------------------------------- 8. boundary expansion and its adjoint
@pytest.mark.parametrize('N,X,L,M', T.DBC_EXPAND_SHAPES)
def test_dbc_expand_forward_and_adjoint_with_channel_slices(N, X, L, M):
    """X = 1 and L = 1 (their embedding is cos(0)), M = 1, N M = 96 (two blocks of the dense reduction); f contiguous and with ldf = M + 4, dout with
    lddo = M + 2 and M + 6."""
    from poisson_cnn_amd import ops
    f, sh, d, dout = T.dbc_inputs(N, X, L, M)
    ref = T.dbc_expand(f, sh, d)
    rdf, rdd = T.dbc_expand_bwd(dout, f, sh, d)
    shd, dd_ = dev(sh), dev(d)
    for fd in (dev(f), framed(f.shape, 2, 4, f)[1]):
        out = host(ops.dbc_expand_fwd(fd, shd, dd_))
        assert out.shape == ref.shape
        e = rel(out[..., :M], ref[..., :M])
        print('dbc_expand %r ldf %d: product channels %.3g' % ((N, X, L, M), ops._ld(fd), e))
        assert e < T.DBC_FWD_TOL
        _check_pos(out, X, L, M)
        for god in (dev(dout), framed(dout.shape, 1, 4, dout)[1]):
            df, dd = ops.dbc_expand_bwd(god, fd, shd, dd_)
            edf, edd = rel(host(df), rdf), rel(host(dd), rdd)
            print('    lddo %d: df %.3g, dd %.3g' % (ops._ld(god), edf, edd))
            assert tuple(df.shape) == (N, 1, L, M) and tuple(dd.shape) == (N, M) and edf < T.DBC_BWD_TOL and edd < T.DBC_BWD_TOL
    buf, view = framed(ref.shape)                                # ldo = M + 5
    ops.handle().call('pcnn_dbc_expand_fwd', c_int(N), c_int(X), c_int(L), c_int(M), ops._p(fd), c_int(ops._ld(fd)), ops._p(shd), ops._p(dd_), ops._p(view),
                      c_int(M + 5))
    assert rel(host(view)[..., :M], ref[..., :M]) < T.DBC_FWD_TOL and np.abs(host(view)[..., M:] - ref[..., M:]).max() <= T.COS_TOL and frame_intact(buf, view)


# ----------------------------------------------------------------------------- 9. per-channel and per-sample forward scaling
@pytest.mark.parametrize('shape', [(3,) + T.SCALE_GRID + (C,) for C in T.SCALE_CHANNELS] + [T.SCALE_BIG])
def test_channel_scale_fwd_and_sample_scale_fwd(shape):
    """C = 1, 3, 32; x dense and a channel slice, the output dense and a channel slice (channel_scale_fwd takes both; sample_scale_fwd takes dense tensors
    only); 3 x 500 x 500 x 3 elements are past the grid cap."""
    from poisson_cnn_amd import ops
    x, s, g = T.scale_inputs(shape)
    ry, rz = T.channel_scale(x, s), T.sample_scale(x, g)
    assert shape != T.SCALE_BIG or x.size > GRID_CAP
    xd = dev(x)
    y = host(ops.channel_scale_fwd(xd, dev(s)))
    assert rel(y, ry) < T.TOL and rel(y[-1, -1, -1], ry[-1, -1, -1]) < T.TOL
    xs = framed(x.shape, 2, 4, x)[1]
    buf, view = framed(x.shape)
    assert ops.channel_scale_fwd(xs, dev(s), out=view) is view
    assert rel(host(view), ry) < T.TOL and frame_intact(buf, view)
    z = host(ops.sample_scale_fwd(xd, dev(g)))
    assert rel(z, rz) < T.TOL and rel(z[-1, -1, -1], rz[-1, -1, -1]) < T.TOL
