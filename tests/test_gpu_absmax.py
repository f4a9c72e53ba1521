"""The absmax side outputs and the hinted split-mode weight gradient (include/pcnn.h: pcnn_conv2d_fwd_absmax, pcnn_conv2d_epilogue_bwd_absmax,
pcnn_conv2d_wgrad_hint).  In the split_f16 math mode the weight gradient scales x and dz by one power of two per tensor, taken from max|x| and
max|dz|; the model never computes those maxima in a pass of their own - every forward convolution and every activation backward emits them as a
by-product and layers.py / models.py hand them on as hints.  A maximum that is too small, stale, or taken from the wrong tensor does not crash, it
costs precision or overflows fp16, so it is pinned here:
  1. y_absmax of every forward route is bit-identical to max|y| of the tensor the kernel stored (dense and channel-sliced, planted maxima at the
     corners of the tile grid, tiny / zero / inf / NaN values),
  2. dz_absmax of both activation-backward kernels likewise,
  3. the hinted weight gradient honours the contract stated in the header (exact hints: bit-identical; hints up to 2^10 too large: same bound;
     inf / NaN hints: clamped; ignored in fp32 mode),
  4. the hints a model hands to its weight gradients describe the tensors they travel with."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_ops, torch_twin

pytestmark = pytest.mark.gpu

TOL = 2e-6        # forward rel-L2 vs the fp64 oracle: the bound of test_gpu_small_conv / test_gpu_conv / test_gpu_spectral(64) / test_gpu_split
TOL_WGRAD = 5e-6  # weight gradient rel-L2 vs fp64 autograd: the bound test_gpu_split (through test_gpu_ops.TOL_RED) applies in split mode
N = 2
PLANT = 50.0


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')


class switches:
    """`with switches(spectral=..., tile=..., xform=..., math=..., limit=...)`: the library's route switches for the enclosed calls, restored afterwards."""

    def __init__(self, spectral='off', tile=0, xform='fft', math='fp32', limit=0):
        self.want = (spectral, tile, xform, math, limit)

    def __enter__(self):
        from poisson_cnn_amd import ops
        self.prev = (ops.get_spectral_mode(), ops.get_spectral_tile(), ops.get_spectral_transform(), ops.get_math_mode())
        self._set(*self.want)

    def __exit__(self, *exc):
        self._set(*self.prev, 0)
        return False

    @staticmethod
    def _set(spectral, tile, xform, math, limit):
        from poisson_cnn_amd import ops
        ops.set_spectral_mode(spectral)
        ops.set_spectral_tile(tile)
        ops.set_spectral_transform(xform)
        ops.set_math_mode(math)
        ops.handle().call('pcnn_set_workspace_limit', ctypes.c_size_t(limit))


# ------------------------------------------------------------------------------------------------------------------ 1. y_absmax of every forward route
# layer: (k, Cin, Cout, H, W, activation);  tile: the (rows, columns) of outputs one workgroup / spectral tile stores;  sw: the switches that force the route;
# same / differ: switch settings under which the same layer must give bit-identical / rounding-different numbers - what shows that the route was taken,
# as in test_gpu_spectral.test_route_is_taken_and_differs_from_direct_only_by_rounding and test_gpu_spectral64.test_tile64_route_is_taken:
#  - the narrow vector-ALU kernels own every 3 x 3 layer of <= 16 channels whatever the switches say and compute the same fp32 FMA chain in both math
#    modes: bit-identical under split_f16 + forced spectral (any MFMA or spectral kernel would differ);
#  - with the spectral route off and > 16 input channels the fp32 mode has only conv_fwd_kernel<NT> (NT = 1 up to 32 output channels, else 2); the split
#    kernel and the spectral kernels give different roundings.  A split-mode call that fell back to the fp32 kernel would be bit-identical to it;
#  - the two transform families, the two tile sizes and the direct kernel all differ from each other by rounding;
#  - <= 16 channels on the spectral route are packed (2 / 4 tiles per work item: cpt < 32) by construction;
#  - the workspace limit: one spectrum item is T^2 x 128 B = 128 KiB (include/pcnn.h), the 7-tap layer below has 2 x 5 x 5 = 50 tiles of 26 x 26 outputs,
#    each with one input and one output item, and a 32-item filter spectrum: 50 x 256 KiB + 4 MiB = 16.5 MiB do not fit the 14 MiB limit, the 32 tiles
#    (12 MiB) that a launch may not go below do - so the layer runs as launches of 32 + 18 tiles (or fails with an error: nothing in between).  A tile's
#    arithmetic does not depend on its launch: bit-identical to the unlimited call.
ROUTES = {
    'narrow_vec':    dict(layer=(3, 8, 8, 19, 40, 'leaky_relu'), tile=(8, 32), vec=True, sw=dict(spectral=-1), same=[dict(spectral='force', math='split_f16')], differ=[]),
    'narrow_scalar': dict(layer=(3, 6, 5, 19, 40, 'tanh'), tile=(8, 32), vec=False, sw=dict(spectral=-1), same=[dict(spectral='force', math='split_f16')], differ=[]),
    'mfma_nt1_vec':  dict(layer=(3, 20, 24, 37, 45, 'leaky_relu'), tile=(16, 32), vec=True, sw=dict(), same=[], differ=[dict(math='split_f16'), dict(spectral='force')]),
    'mfma_nt1_scalar': dict(layer=(3, 20, 23, 37, 45, 'leaky_relu'), tile=(16, 32), vec=False, sw=dict(), same=[], differ=[dict(math='split_f16'), dict(spectral='force')]),
    'mfma_nt2':      dict(layer=(3, 24, 40, 37, 45, 'tanh'), tile=(16, 32), vec=True, sw=dict(), same=[], differ=[dict(math='split_f16')]),
    'split':         dict(layer=(3, 20, 24, 37, 45, 'leaky_relu'), tile=(8, 32), vec=True, sw=dict(math='split_f16'), same=[], differ=[dict()]),
    'spec32_mfma':   dict(layer=(7, 32, 20, 45, 53, 'leaky_relu'), tile=(26, 26), vec=True, sw=dict(spectral='force', tile=32, xform='mfma'), same=[],
                          differ=[dict(spectral='force', tile=32, xform='fft'), dict()]),
    'spec32_fft':    dict(layer=(7, 32, 20, 45, 53, 'tanh'), tile=(26, 26), vec=True, sw=dict(spectral='force', tile=32, xform='fft'), same=[],
                          differ=[dict(spectral='force', tile=32, xform='mfma'), dict()]),
    'spec32_packed': dict(layer=(9, 8, 8, 45, 53, 'leaky_relu'), tile=(24, 24), vec=True, sw=dict(spectral='force', tile=32, xform='fft'), same=[],
                          differ=[dict(spectral='force', tile=32, xform='mfma'), dict()]),
    'spec32_limit':  dict(layer=(7, 32, 20, 110, 110, 'leaky_relu'), tile=(26, 26), vec=True, sw=dict(spectral='force', tile=32, xform='fft', limit=14 << 20),
                          same=[dict(spectral='force', tile=32, xform='fft')], differ=[dict()]),
    'spec64_mfma':   dict(layer=(13, 28, 28, 75, 70, 'leaky_relu'), tile=(52, 52), vec=True, sw=dict(spectral='force', tile=64, xform='mfma'), same=[],
                          differ=[dict(spectral='force', tile=32, xform='mfma')]),
    'spec64_fft':    dict(layer=(13, 28, 28, 75, 70, 'leaky_relu'), tile=(52, 52), vec=True, sw=dict(spectral='force', tile=64, xform='fft'), same=[],
                          differ=[dict(spectral='force', tile=32, xform='fft')]),
}
PAD_MODE = 'SYMMETRIC'
_layers = {}     # layer -> host data and the fp64 reference without the residual (computed once, never modified)


def layer_data(layer):
    """Everything of a case that does not depend on the planted entry: operands as float32-representable fp64 arrays and
    base = act(conv(x) + b) * bn_scale + bn_shift in fp64 (oracle.np_ops.padded_conv2d), NCHW."""
    if layer not in _layers:
        k, Cin, Cout, H, W, act = layer
        rng = np.random.default_rng(1000 * k + 31 * Cin + Cout + H)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        x = f32(rng.standard_normal((N, Cin, H, W)))
        w = f32(rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin))
        b = f32(rng.standard_normal(Cout))
        sc, sh = f32(rng.uniform(0.5, 1.5, Cout)), f32(rng.standard_normal(Cout))
        res = f32(rng.standard_normal((N, Cout, H, W)))
        a = np_ops.padded_conv2d(x, w, b, PAD_MODE, 0.0, act)
        base = a * sc[None, :, None, None] + sh[None, :, None, None]
        _layers[layer] = dict(x=x, w=w, b=b, sc=sc, sh=sh, res=res, a=a, base=base)
    return _layers[layer]


def planted_position(route, which):
    k, Cin, Cout, H, W, act = ROUTES[route]['layer']
    ty, tx = ROUTES[route]['tile']
    return [(0, 0, 0, 0),
            (N - 1, H - 1, W - 1, Cout - 1),
            (N - 1, (H // ty) * ty - 1, (W // tx) * tx - 1, Cout // 2),      # the last pixel of the last full tile: its neighbours below / right are ragged
            (0, H // 2, W // 2, 4 * ((Cout - 1) // 4))][which]               # the first channel of the last (possibly partial) channel quad


def planted_reference(route, which, sign):
    """(residual NCHW with the planted entry, fp64 reference NCHW, position)."""
    d = layer_data(ROUTES[route]['layer'])
    n, y, x, c = planted_position(route, which)
    res = d['res'].copy()
    res[n, c, y, x] = sign * PLANT
    return res, d['base'] + res, (n, y, x, c)


def launch(route, sw, res, sliced, prefill=1e30, use_bias=True, use_bn=True, x_scale=None):
    """One forward call of the route's layer under the switches `sw`.  Returns (the wide output buffer, the view the kernel wrote, act_out, y_absmax)."""
    from poisson_cnn_amd import ops
    k, Cin, Cout, H, W, act = ROUTES[route]['layer']
    d = layer_data(ROUTES[route]['layer'])
    vec = ROUTES[route]['vec']
    off, tail = ((4, 4) if vec else (1, 2)) if sliced else (0, 0)           # vector routes keep 16-byte aligned quads in the slice, scalar ones lose them
    xd = dev(d['x'].transpose(0, 2, 3, 1))
    if x_scale is not None:
        xd = xd * x_scale
    outb = torch.zeros((N, H, W, off + Cout + tail), dtype=torch.float32, device='cuda')
    out = outb[..., off:off + Cout]
    a_out = torch.empty((N, H, W, Cout), dtype=torch.float32, device='cuda')
    amax = torch.full((1,), prefill, dtype=torch.float32, device='cuda')
    p = np_ops.advanced_pad_amounts(k)[0]
    with switches(**sw):
        ops.conv2d_fwd(xd, dev(d['w']), dev(d['b']) if use_bias else None, pad_top=p, pad_left=p, pad_mode=PAD_MODE, act=act,
                       bn_scale=dev(d['sc']) if use_bn else None, bn_shift=dev(d['sh']) if use_bn else None,
                       residual=dev(res.transpose(0, 2, 3, 1)) if res is not None else None, out=out, act_out=a_out, y_absmax=amax)
        torch.cuda.synchronize()
    return outb, out, a_out, amax


_route_checked = {}


def check_route_is_taken(route):
    """Once per route (the outcome is kept): the same layer under the route's own switches and under the `same` / `differ` settings."""
    if route not in _route_checked:
        r = ROUTES[route]
        res = layer_data(r['layer'])['res']
        y0 = launch(route, r['sw'], res, False)[1]
        msgs = []
        for sw in r['same']:
            if not torch.equal(launch(route, sw, res, False)[1], y0):
                msgs.append('%s: not bit-identical under %r' % (route, sw))
        for sw in r['differ']:
            y1 = launch(route, sw, res, False)[1]
            e = rel(y1.cpu().numpy(), y0.cpu().numpy())
            if not 0 < e < 1e-5:
                msgs.append('%s: rel. difference %g to the same layer under %r (expected: rounding, not zero)' % (route, e, sw))
        _route_checked[route] = msgs
    assert not _route_checked[route], _route_checked[route]


def test_planted_maximum_is_the_reference_maximum_for_every_case():
    """Host only: the fp64 reference alone puts its global maximum at the planted position, so the bit-identity below is about that entry."""
    for route in ROUTES:
        for which in range(4):
            for sign in (1.0, -1.0):
                _, ref, (n, y, x, c) = planted_reference(route, which, sign)
                assert np.unravel_index(np.argmax(np.abs(ref)), ref.shape) == (n, c, y, x), (route, which, sign)
                assert np.sort(np.abs(ref).ravel())[-2] < 0.6 * np.abs(ref[n, c, y, x])


@pytest.mark.parametrize('sign', [1.0, -1.0])
@pytest.mark.parametrize('which', [0, 1, 2, 3], ids=['first', 'last', 'tile_edge', 'last_quad'])
@pytest.mark.parametrize('sliced', [False, True], ids=['dense', 'slice'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_forward_absmax_is_the_maximum_of_what_was_stored(route, sliced, which, sign):
    r = ROUTES[route]
    k, Cin, Cout, H, W, act = r['layer']
    check_route_is_taken(route)
    res, ref, (n, y, x, c) = planted_reference(route, which, sign)
    outb, out, a_out, amax = launch(route, r['sw'], res, sliced)
    got = out.cpu().numpy().transpose(0, 3, 1, 2)
    print('%s: y_absmax %r, max|out| %r, rel-L2 vs fp64 %.3g' % (route, float(amax), float(out.abs().max()), rel(got, ref)))
    assert torch.equal(amax, out.abs().max().reshape(1)), (float(amax), float(out.abs().max()))       # overwritten (not 1e30), and the very float that was stored
    assert rel(got, ref) < TOL and rel(a_out.cpu().numpy().transpose(0, 3, 1, 2), layer_data(r['layer'])['a']) < TOL
    assert np.unravel_index(np.argmax(np.abs(got)), got.shape) == (n, c, y, x)
    if sliced:
        lo = out.storage_offset() - outb.storage_offset()
        assert float(outb[..., :lo].abs().max()) == 0.0 and float(outb[..., lo + Cout:].abs().max()) == 0.0


@pytest.mark.parametrize('route', ['narrow_vec', 'narrow_scalar', 'spec32_fft'])
def test_forward_absmax_edge_values(route):
    r = ROUTES[route]
    d = layer_data(r['layer'])
    check_route_is_taken(route)
    # outputs of ~1e-30: small normal floats order like their bit patterns, too
    outb, out, _, amax = launch(route, r['sw'], d['res'] * 1e-30, False, use_bias=False, use_bn=False, x_scale=1e-30)
    assert torch.equal(amax, out.abs().max().reshape(1)) and 1e-32 < float(amax) < 1e-28
    # an all-zero output: exactly 0.0 (and not the 1e30 that was there before)
    outb, out, _, amax = launch(route, r['sw'], None, False, use_bias=False, use_bn=False, x_scale=0.0)
    assert float(out.abs().max()) == 0.0 and float(amax) == 0.0
    # one +inf: the side output stays a finite scale (3.0e38), the tensor carries the inf
    k, Cin, Cout, H, W, act = r['layer']
    res = d['res'].copy()
    res[1, Cout - 1, H // 2, W - 1] = np.inf
    outb, out, _, amax = launch(route, r['sw'], res, False)
    assert bool(torch.isinf(out).any()) and torch.equal(amax, torch.tensor([3.0e38], dtype=torch.float32, device='cuda'))
    # one NaN: ignored by the maximum (fmaxf), which is then the maximum of the other entries
    res[1, Cout - 1, H // 2, W - 1] = np.nan
    outb, out, _, amax = launch(route, r['sw'], res, False)
    assert bool(torch.isnan(out).any()) and bool(torch.isfinite(amax).all())
    assert torch.equal(amax, torch.nan_to_num(out, nan=0.0).abs().max().reshape(1))


# ------------------------------------------------------------------------------------------------------------------ 2. dz_absmax of the activation backward
EPI_FORMS = {'vec4': (8, 0, 8), 'generic_c6': (6, 0, 6), 'generic_slice': (8, 1, 12)}     # C, first channel of dy in its buffer, that buffer's width


@pytest.mark.parametrize('last', [False, True], ids=['first_pixel', 'last_pixel'])
@pytest.mark.parametrize('bn', [False, True], ids=['plain', 'bn_scale'])
@pytest.mark.parametrize('act', ['leaky_relu', 'tanh'])
@pytest.mark.parametrize('form', list(EPI_FORMS))
def test_epilogue_bwd_absmax(form, act, bn, last):
    """dz = dy * bn_scale * act'(a) (include/pcnn.h, pcnn_conv2d_epilogue_bwd) and max|dz| of what was stored: the float4 kernel and the generic one
    (ragged channel count; dy as a channel slice that starts at channel 1), 2 x 19 x 23 pixels (no multiple of the rows per workgroup)."""
    from poisson_cnn_amd import ops
    C, first, width = EPI_FORMS[form]
    H, W = 19, 23
    rng = np.random.default_rng(7 * C + first)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    dy = f32(rng.standard_normal((N, H, W, C)))
    a = f32(rng.standard_normal((N, H, W, C)))
    if act == 'tanh':
        a = f32(np.tanh(a))
    sc = f32(rng.uniform(0.5, 1.5, C)) if bn else None
    pix = (N - 1, H - 1, W - 1) if last else (0, 0, 0)
    cpl = C - 1 if last else 0
    dy[pix + (cpl,)] = -40.0 if last else 40.0
    a[pix + (cpl,)] = 0.125                                    # slope 1 (leaky ReLU) / 1 - 2^-6 (tanh): the planted entry stays the maximum
    grad = np.where(a > 0, 1.0, 0.2) if act == 'leaky_relu' else 1.0 - a * a
    ref = dy * (sc if bn else 1.0) * grad
    assert np.unravel_index(np.argmax(np.abs(ref)), ref.shape) == pix + (cpl,)
    dyb = torch.zeros((N, H, W, width), dtype=torch.float32, device='cuda')
    dyd = dyb[..., first:first + C]
    dyd.copy_(dev(dy))
    dz = torch.empty((N, H, W, C), dtype=torch.float32, device='cuda')
    db = torch.empty((C,), dtype=torch.float32, device='cuda')
    t = torch.full((1,), 1e30, dtype=torch.float32, device='cuda')
    ops.epilogue_bwd(dyd, dev(a), act=act, bn_scale=dev(sc) if bn else None, dz=dz, dbias=db, dz_absmax=t)
    torch.cuda.synchronize()
    assert torch.equal(t, dz.abs().max().reshape(1)), (float(t), float(dz.abs().max()))
    assert rel(dz.cpu().numpy(), ref) < TOL                    # the bound of test_gpu_ops.test_epilogue_bwd_and_bn_fold
    assert rel(db.cpu().numpy(), ref.sum((0, 1, 2))) < 5e-6
    # the linear layer with a bias (dz is dy itself: not written) still reports max|dy * scale|
    t2 = torch.full((1,), 1e30, dtype=torch.float32, device='cuda')
    scd = dev(sc) if bn else None
    assert ops.epilogue_bwd(dyd, None, act='linear', bn_scale=scd, dz=None, dbias=db, dz_absmax=t2) is None
    want = (dyd * scd if bn else dyd).abs().max().reshape(1)
    assert torch.equal(t2, want), (float(t2), float(want))


# ------------------------------------------------------------------------------------------------------------------ 3. the hinted weight gradient
# > 16 channels on one side: the narrow vector-ALU weight gradient owns 3 x 3 / 5 x 5 layers of <= 16 channels in both math modes and takes no hints.
# All four shapes pass split_eligible (one output channel group, <= 4 MFMA taps per wave); 37 x 45 leaves a ragged last 8 x 32 tile in both axes.
WGRAD_CASES = [(3, 20, 24, 'CONSTANT', False), (5, 24, 20, 'SYMMETRIC', False), (3, 20, 24, 'REFLECT', True), (3, 18, 21, 'CONSTANT', False)]


@pytest.mark.parametrize('k,Cin,Cout,pad_mode,sliced', WGRAD_CASES)
def test_hinted_weight_gradient_honours_its_contract(k, Cin, Cout, pad_mode, sliced):
    """The header's 'within a factor 2^10' holds at the bound the unhinted split-mode weight gradient is held to (5e-6), with room: measured rel-L2 of
    dw against fp64 autograd on an MI355X, hints = factor x the exact maxima of both tensors - factor 1: 2.01e-7, 2^5: 2.01e-7, 2^10: 2.01e-7
    (3x3 20 -> 24 CONSTANT; 1.9e-7 ... 2.0e-7 for the other three cases, 2^10 on one tensor alone included).  The figures are printed on every run."""
    from poisson_cnn_amd import ops
    rng = np.random.default_rng(100 * k + Cin + Cout)
    H, W = 37, 45
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    x, dz = f32(rng.standard_normal((N, Cin, H, W))), f32(rng.standard_normal((N, Cout, H, W)))
    xt, wt = torch.tensor(x), torch.zeros((k, k, Cin, Cout), dtype=torch.float64, requires_grad=True)
    (torch_twin.padded_conv2d(xt, wt, None, pad_mode, 0.3, 'linear') * torch.tensor(dz)).sum().backward()
    ref = wt.grad.numpy()
    p = k // 2

    def on_device(a, C):
        if not sliced:
            return dev(a.transpose(0, 2, 3, 1))
        buf = torch.randn((N, H, W, C + 8), dtype=torch.float32, device='cuda') * 100.0    # neighbours of the slice: larger than anything inside it
        buf[..., 4:4 + C].copy_(dev(a.transpose(0, 2, 3, 1)))
        return buf[..., 4:4 + C]

    xd, dzd = on_device(x, Cin), on_device(dz, Cout)
    scalar = lambda v: torch.tensor([v], dtype=torch.float32, device='cuda')

    def wgrad(xa=xd, za=dzd, pad_value=0.3, **hints):
        dw = ops.conv2d_wgrad(xa, za, (k, k, Cin, Cout), pad_top=p, pad_left=p, pad_mode=pad_mode, pad_value=pad_value, **hints)
        torch.cuda.synchronize()
        return dw

    mx, mz = float(xd.abs().max()), float(dzd.abs().max())
    with switches(math='fp32'):
        f0 = wgrad()
        assert torch.equal(wgrad(x_absmax=scalar(mx), dz_absmax=scalar(mz)), f0)
        assert torch.equal(wgrad(x_absmax=scalar(1e-20), dz_absmax=scalar(float('inf'))), f0)     # ignored in fp32 mode, however wrong
        assert rel(f0.cpu().numpy(), ref) < TOL_WGRAD
    with switches(math='split_f16'):
        s0 = wgrad()
        assert not torch.equal(s0, f0), 'the split kernel did not run'
        assert rel(s0.cpu().numpy(), ref) < TOL_WGRAD
        assert torch.equal(wgrad(x_absmax=scalar(mx), dz_absmax=scalar(mz)), s0)            # the same maxbits either way
        errs = {}
        for fx, fz in ((1.0, 1.0), (32.0, 32.0), (1024.0, 1.0), (1.0, 1024.0), (1024.0, 1024.0)):
            errs[(fx, fz)] = rel(wgrad(x_absmax=scalar(fx * mx), dz_absmax=scalar(fz * mz)).cpu().numpy(), ref)
        print('k=%d %d->%d %s: dw rel-L2 vs fp64 by hint factor (x, dz):' % (k, Cin, Cout, pad_mode), {kk: '%.3g' % v for kk, v in errs.items()})
        assert max(errs.values()) < TOL_WGRAD, errs
        for bad in (float('inf'), float('nan')):                                            # clamped by split_absmax_kernel: the scale stays finite
            assert bool(torch.isfinite(wgrad(x_absmax=scalar(bad), dz_absmax=scalar(bad))).all())
        # the per-tensor scale is the point of the mode: operands 24 orders of magnitude apart (x * 9.1e-13, dz * 1.1e+12 - powers of two, so that the
        # scaled float32 operands, the scaled padding constant and with them the fp64 reference are exact)
        xs, zs = xd * 2.0 ** -40, dzd * 2.0 ** 40
        hx, hz = xs.abs().max().reshape(1), zs.abs().max().reshape(1)
        dws = wgrad(xs, zs, pad_value=float(np.float32(0.3)) * 2.0 ** -40, x_absmax=hx, dz_absmax=hz)
        assert rel(dws.cpu().numpy(), ref) < TOL_WGRAD
        if pad_mode == 'CONSTANT':
            # a padding constant far above max|x| (0.3 beside 4e-12) goes through x's scale into the fp16 halves as well: it has to take part in that
            # scale, with and without a hint (it did not: 0.3 * 2^50 overflowed the halves and every entry of dw was NaN).  dw is linear in the
            # padded input: the image's part (the gradient under zero padding) scales with x, the padding's part does not
            w0 = torch.zeros((k, k, Cin, Cout), dtype=torch.float64, requires_grad=True)
            (torch_twin.padded_conv2d(xt, w0, None, pad_mode, 0.0, 'linear') * torch.tensor(dz)).sum().backward()
            ref_pad = ref - w0.grad.numpy()
            want = w0.grad.numpy() * 2.0 ** -40 + ref_pad
            for hints in (dict(), dict(x_absmax=hx, dz_absmax=scalar(mz))):
                dwp = wgrad(xs, dzd, **hints)
                assert rel(dwp.cpu().numpy(), want) < TOL_WGRAD, hints


# ------------------------------------------------------------------------------------------------------------------ 4. the hints inside a model
def record_wgrad_calls(monkeypatch):
    """Wraps ops.conv2d_wgrad (the layers call it through the module): before delegating, keeps max|x|, max|dz| and the hints as device values."""
    from poisson_cnn_amd import ops
    calls = []
    real = ops.conv2d_wgrad

    def wrapper(x, dz, w_shape, **kw):
        xa, za = kw.get('x_absmax'), kw.get('dz_absmax')
        calls.append((tuple(w_shape), x.abs().max(), dz.abs().max(), xa.clone() if xa is not None else None, za.clone() if za is not None else None))
        return real(x, dz, w_shape, **kw)

    monkeypatch.setattr(ops, 'conv2d_wgrad', wrapper)
    return calls


def check_hints(calls):
    torch.cuda.synchronize()
    nx = nz = 0
    for w_shape, mx, mz, hx, hz in calls:
        for m, h in ((mx, hx), (mz, hz)):
            if h is not None:
                m, h = float(m), float(h)
                assert m <= h <= 2.0 ** 10 * m, 'layer %r: max|t| = %r, hint = %r' % (w_shape, m, h)
        nx += hx is not None
        nz += hz is not None
    return nx, nz


def conv_units(obj, seen=None, depth=0):
    """Every layers.ConvUnit reachable from a model's attributes."""
    from poisson_cnn_amd import layers as L
    seen = set() if seen is None else seen
    if id(obj) in seen or depth > 8:
        return []
    seen.add(id(obj))
    if isinstance(obj, L.ConvUnit):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [u for o in obj for u in conv_units(o, seen, depth + 1)]
    if isinstance(obj, dict):
        return [u for o in obj.values() for u in conv_units(o, seen, depth + 1)]
    if type(obj).__module__.startswith('poisson_cnn_amd') and hasattr(obj, '__dict__'):
        return [u for o in vars(obj).values() for u in conv_units(o, seen, depth + 1)]
    return []


def test_model_hints_describe_the_tensors_they_travel_with(monkeypatch):
    from poisson_cnn_amd import configs
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    from poisson_cnn_amd.train import SGD
    full = configs.hpnn_tiny()
    rng = np.random.default_rng(11)
    rhs = rng.uniform(-1, 1, (2, 1, 44, 38)).astype(np.float32)
    dx = rng.uniform(5e-3, 5e-2, (2, 1)).astype(np.float32)
    tgt = (rng.standard_normal(rhs.shape) * 0.1).astype(np.float32)
    with switches(spectral=-1, math='split_f16'):
        model = Homogeneous_Poisson_NN_Legacy(**full['model'], seed=3)
        model.compile(loss=loss_wrapper(global_batch_size=2, **full['training']['loss_parameters']), optimizer=SGD(learning_rate=0.0))
        calls = record_wgrad_calls(monkeypatch)
        model.train_step(((rhs, dx), tgt))
        nx, nz = check_hints(calls)
        assert nx > 0 and nz > 0, 'no weight gradient of the step carried a hint (x: %d, dz: %d of %d calls)' % (nx, nz, len(calls))
        units = conv_units(model)
        ran = [u for u in units if hasattr(u, 'out_absmax')]
        assert len(ran) > 10
        missing = [u.name for u in ran if u.stride == 1 and u.out_absmax is None]
        assert not missing, missing


def _standalone(build):
    from poisson_cnn_amd import layers as L
    S, C = L.ParamStore(), L.Context()
    obj = build(S, C)
    S.finalize('cuda')
    S.initialize(5)
    for name in S.w:
        if name.endswith('/bias'):
            S.w[name].normal_()
    return obj


def test_layer_hint_with_a_sliced_input_and_two_calls_per_step(monkeypatch):
    from poisson_cnn_amd import layers as L
    with switches(spectral='off', math='split_f16'):
        u = _standalone(lambda S, C: L.ConvUnit(S, C, 'u', 3, 20, 24, activation='leaky_relu'))
        g = torch.Generator(device='cuda').manual_seed(1)
        wide = torch.randn(2, 37, 45, 28, device='cuda', generator=g)
        wide[..., :4] *= 100.0
        y1 = u.forward(wide[..., 4:24], training=True)
        h1 = u.out_absmax
        assert h1 is not None and torch.equal(h1, y1.abs().max().reshape(1))
        y2 = u.forward(wide[..., 4:24] * 3.0, training=True)                           # a second call in the same step
        h2 = u.out_absmax
        assert h2 is not None and h2.data_ptr() != h1.data_ptr(), 'a fresh buffer per call'
        torch.cuda.synchronize()
        assert torch.equal(h1, y1.abs().max().reshape(1)) and torch.equal(h2, y2.abs().max().reshape(1))
        calls = record_wgrad_calls(monkeypatch)
        u.forward(wide[..., 4:24], training=True, x_absmax=wide[..., 4:24].abs().max().reshape(1))
        u.backward(torch.randn(2, 37, 45, 24, device='cuda', generator=g), need_dx=False)
        assert check_hints(calls) == (1, 1)


def test_resnet_stage_hints_include_the_residual(monkeypatch):
    """layers.resnet: c0 -> c1 (+ x) -> c2.  c2's input is c1's output WITH the skip connection: its hint must be the maximum after the add."""
    from poisson_cnn_amd import layers as L
    with switches(spectral='off', math='split_f16'):                                   # (off: every weight gradient of the stage goes through ops.conv2d_wgrad)
        r = _standalone(lambda S, C: L.resnet(S, C, 'r', 20, 3, activation='leaky_relu'))
        g = torch.Generator(device='cuda').manual_seed(2)
        x = torch.randn(2, 37, 45, 20, device='cuda', generator=g)
        x[1, 36, 44, 19] = -50.0                                                       # the skip connection carries the maximum of c2's input
        xmax = x.abs().max().reshape(1)
        calls = record_wgrad_calls(monkeypatch)
        y = r.forward(x, training=True, x_absmax=xmax)
        assert r.out_absmax is not None and torch.equal(r.out_absmax, y.abs().max().reshape(1))
        c2_in = r.c2.saved[0]
        assert float(c2_in.abs().max()) >= 40.0 and torch.equal(r.c1.out_absmax, c2_in.abs().max().reshape(1))
        assert torch.equal(r.c0.out_absmax, r.c1.saved[0].abs().max().reshape(1))
        r.backward(torch.randn(2, 37, 45, 20, device='cuda', generator=g))
        r.c0.ctx.join()
        nx, nz = check_hints(calls)
        assert len(calls) == 3 and nx == 3 and nz >= 1, (len(calls), nx, nz)
