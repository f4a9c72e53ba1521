"""Every convolution route with rectangular filters (kh != kw), unequal offsets (pad_top != pad_left), VALID geometry, pads at the tf.pad
limit, ragged channel counts and channel-slice views, against the geometry-general fp64 reference of tests/conv_geometry.py.

Routes (selected with the library's own setters, restored afterwards; proved taken by a result that differs from the neighbouring route's by
more than 0 and less than the tolerance):

    direct        spectral off, fp32 MFMA implicit GEMM (conv_fwd.hip, conv_wgrad.hip)
    split         spectral off, 3 x fp16 split MFMA (conv_fwd_split.hip, the split weight gradient)
    spec32-mfma   spectral forced, 32-point tiles, DFT on the matrix cores (spectral_conv.hip)
    spec32-fft    spectral forced, 32-point tiles, in-register FFTs (spectral_fft.hip)
    spec64-mfma   spectral forced, 64-point tiles (spectral64.hip)
    spec64-fft    spectral forced, 64-point tiles, FFT transforms

Operations per case and route: forward (bias; BN affine + residual + act_out on the slice rows), data gradient (flipped filter; padded-domain
form + pad_fold_bwd for SYMMETRIC / REFLECT), weight gradient (twice, bitwise equal) and, on the spectral routes, the fused backward (twice,
bitwise equal; with `residual` for CONSTANT; once per tile size with a Post).

A route that does not take a case hands it to another kernel, and the result is then bit-identical to that kernel's: such a case is COUNTED as
declined in the ledger (it was already asserted on the kernel that ran it).  The last test of the module asserts that every (case kind, route,
operation) cell ran at least one case and that no route declined more than a quarter of its cases.  One exception, by arithmetic: pick_tile
gives 64-point tiles only to filters with both sides >= 9, and 7 of the 14 filters of the table have a side below 9.  Those cases are still
run with tile 64 forced (forward: must be bit-identical to the 32-point result) and counted apart as `below64`; the quarter cap of the two
64-point routes is taken over the cases with both sides >= 9, and each case kind has at least one such case.

Bounds.  Whole tensor: rel-L2 <= 2e-6 forward and data gradient, <= 5e-6 weight and bias gradient (tests/test_gpu_conv.py,
tests/test_gpu_ops.py; tests/test_gpu_split.py uses the same for the split mode).  Direct fp32 route: additionally element-wise
|y - ref| <= gamma(K) (|x| (*) |w| + |b|) on the pre-activation (linear rows), K = kh kw Cin + 1 forward, kh kw Cout (+ 3 for the at most four
padded positions that fold onto one pixel) data gradient, N Ho Wo weight gradient: derived (Higham 3.1), no margin.  Spectral routes: the same
rel-L2 bounds on every region of conv_geometry.regions (border band, each output channel, each sample).

Region bounds that differ from 2e-6 / 5e-6: none (REGION_BOUNDS is empty).  Measured on an MI355X, worst case of the table as a fraction of
its bound - so no region needed the float32-CPU procedure (a bound of max(project bound, 4 x the same region's error of a float32 CPU
convolution against the fp64 reference), which is how an entry of REGION_BOUNDS would have to be derived):

    route         fwd whole / region   dgrad whole / region   wgrad whole / region   fused dx / dw (region)   element-wise (direct only)
    direct        0.10  / -            0.13  / -              0.06  / -              -                        fwd 0.012  dgrad 0.017  wgrad 0.002
    split         0.20  / -            0.22  / -              0.05  / -              -
    spec32-mfma   0.13  / 0.18         0.15  / 0.15           0.06  / 0.07           0.13 / 0.06
    spec32-fft    0.13  / 0.17         0.14  / 0.14           0.05  / 0.05           0.12 / 0.05
    spec64-mfma   0.14  / 0.18         0.14  / 0.15           0.06  / 0.07           0.13 / 0.06
    spec64-fft    0.12  / 0.18         0.13  / 0.14           0.05  / 0.05           0.12 / 0.05

Declined (of 63 cases; 24 with both filter sides >= 9 for the 64-point routes): spectral forward 3 (Cout = 33), spectral and split weight
gradient and the fused backward 6 (Cout = 64 and 33), 64-point tiles additionally the packed 3 -> 4 layer.  Sensitivity test: a correct result
with one of 32 channels scaled by 1 + 8e-6 has whole-tensor error 1.0e-6 .. 1.1e-6 (passes 2e-6) and per-channel error 7.9e-6 .. 8.0e-6
(rejected) on all six routes; the kernels' own error there is 1.4e-7 .. 2.3e-7.  Wall time of this module on the MI355X: 15 s.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import conv_geometry as G
from oracle import np_ops

pytestmark = pytest.mark.gpu

TOL, TOL_RED = 2e-6, 5e-6
PAD_VALUE = float(np.float32(0.3))
ROUTES = ('direct', 'split', 'spec32-mfma', 'spec32-fft', 'spec64-mfma', 'spec64-fft')
SPECTRAL = ROUTES[2:]
FALLBACK = {'split': 'direct', 'spec32-mfma': 'direct', 'spec32-fft': 'direct', 'spec64-mfma': 'spec32-mfma', 'spec64-fft': 'spec32-fft'}
NEIGHBOUR = {'split': 'direct', 'spec32-mfma': 'direct', 'spec32-fft': 'spec32-mfma', 'spec64-mfma': 'spec32-mfma', 'spec64-fft': 'spec64-mfma'}
KINDS = ('odd/odd', 'even/odd', 'tile64 boundary', 'offsets', 'valid', 'pad limit', 'channels', 'slices')
# (region, operation) -> bound where it differs from the project's; filled only by the procedure of the module docstring
#   region | operation | float32 CPU convolution, same region | bound
#   (none)
REGION_BOUNDS = {}

LEDGER = {}          # (kind, route, op) -> [ran, declined]
BELOW64 = {}         # route -> cases with a filter side below 9 (run, bit-identical to the 32-point tiles)
FIGURES = {}         # (route, op) -> worst figure / bound seen


def note(kind, route, op, declined):
    LEDGER.setdefault((kind, route, op), [0, 0])[1 if declined else 0] += 1


def figure(route, op, value, bound):
    FIGURES[(route, op)] = max(FIGURES.get((route, op), 0.0), value / bound)


@contextlib.contextmanager
def selected(route):
    """The route's switches, set through the public setters; the previous values come back whatever happens inside."""
    from poisson_cnn_amd import ops
    prev = (ops.get_spectral_mode(), ops.get_spectral_tile(), ops.get_spectral_transform(), ops.get_math_mode())
    try:
        ops.set_math_mode('split_f16' if route == 'split' else 'fp32')
        if route in ('direct', 'split'):
            ops.set_spectral_mode('off')
        else:
            ops.set_spectral_mode('force')
            ops.set_spectral_tile(64 if route.startswith('spec64') else 32)
            ops.set_spectral_transform(route.split('-')[1])
        yield
    finally:
        ops.set_spectral_mode(prev[0]); ops.set_spectral_tile(prev[1]); ops.set_spectral_transform(prev[2]); ops.set_math_mode(prev[3])


@pytest.fixture(autouse=True)
def switches_restored():
    from poisson_cnn_amd import ops
    prev = (ops.get_spectral_mode(), ops.get_spectral_tile(), ops.get_spectral_transform(), ops.get_math_mode())
    yield
    assert (ops.get_spectral_mode(), ops.get_spectral_tile(), ops.get_spectral_transform(), ops.get_math_mode()) == prev
    os.environ.pop('PCNN_GROUPED_VALU', None)


# ------------------------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, kind, kh, kw, mode, act, H, W, Cin, Cout, pt=None, pl=None, out_hw=None, slices=False):
        self.kind, self.kh, self.kw, self.mode, self.act, self.H, self.W, self.Cin, self.Cout = kind, kh, kw, mode, act, H, W, Cin, Cout
        self.pt = kh // 2 if pt is None else pt
        self.pl = kw // 2 if pl is None else pl
        self.Ho, self.Wo = out_hw if out_hw is not None else (H, W)
        self.slices = slices
        (_, self.pb), (_, self.pr) = G.pads_of(H, W, kh, kw, self.pt, self.pl, (self.Ho, self.Wo))
        self.can64 = kh >= 9 and kw >= 9
        self.id = '%s-%dx%d-%s-%s-%dx%d-%dto%d-p%d.%d%s' % (kind.replace(' ', '_').replace('/', '_'), kh, kw, mode[:3], act[:4], H, W, Cin, Cout,
                                                          self.pt, self.pl, '-slices' if slices else '')


def _size(kh, kw):
    """Images with at least two tiles per axis and an overhanging last tile on every route that can take the filter: 60 x 62 covers two 64-point
    tiles (valid region 65 - k >= 50) and four 32-point ones; filters with a side below 9 never see 64-point tiles: 40 x 45 covers two 32-point
    tiles (valid region 33 - k >= 18)."""
    return (60, 62, 18, 6) if (kh >= 9 and kw >= 9) else (40, 45, 6, 5)


def _cases():
    acts = ('leaky_relu', 'tanh', 'linear')
    modes = ('CONSTANT', 'SYMMETRIC', 'REFLECT')
    out = []
    rect = [('odd/odd', f) for f in ((3, 7), (7, 3), (15, 9), (9, 15), (13, 5))] + [('even/odd', f) for f in ((4, 13), (13, 4), (2, 15), (6, 11), (10, 13))]
    for i, (kind, (kh, kw)) in enumerate(rect):
        for j, mode in enumerate(modes):
            H, W, Cin, Cout = _size(kh, kw)
            if j == 2 and not (kh >= 9 and kw >= 9):
                Cin, Cout = 20, 12                       # one full 32-lane tile per work item instead of packed tiles
            out.append(Case(kind, kh, kw, mode, acts[(i + j) % 3], H, W, Cin, Cout))
    for (kh, kw), mode, act in (((14, 15), 'CONSTANT', 'leaky_relu'), ((15, 13), 'SYMMETRIC', 'tanh'), ((8, 15), 'REFLECT', 'linear')):
        out.append(Case('tile64 boundary', kh, kw, mode, act, 60, 62, 18, 6))
    # unequal offsets: pb = Ho - H + kh - 1 - pad_top, pr = Wo - W + kw - 1 - pad_left, all >= 0
    out.append(Case('offsets', 7, 7, 'CONSTANT', 'linear', 40, 45, 6, 5, pt=1, pl=5, out_hw=(38, 46)))
    out.append(Case('offsets', 5, 9, 'SYMMETRIC', 'tanh', 40, 45, 6, 5, pt=4, pl=0, out_hw=(41, 40)))
    out.append(Case('offsets', 11, 13, 'CONSTANT', 'leaky_relu', 60, 62, 18, 6, pt=2, pl=9, out_hw=(57, 64)))
    out.append(Case('valid', 5, 9, 'CONSTANT', 'leaky_relu', 40, 45, 6, 5, pt=0, pl=0, out_hw=(36, 37)))
    out.append(Case('valid', 11, 3, 'SYMMETRIC', 'tanh', 40, 45, 6, 5, pt=0, pl=0, out_hw=(30, 43)))
    out.append(Case('valid', 13, 9, 'CONSTANT', 'linear', 70, 72, 18, 6, pt=0, pl=0, out_hw=(58, 64)))
    # pads at the tf.pad limit: SYMMETRIC size = k // 2, REFLECT size = k // 2 + 1, in y and then in x
    out.append(Case('pad limit', 15, 9, 'SYMMETRIC', 'linear', 7, 62, 18, 6))
    out.append(Case('pad limit', 15, 9, 'REFLECT', 'leaky_relu', 8, 62, 18, 6))
    out.append(Case('pad limit', 9, 15, 'SYMMETRIC', 'tanh', 60, 7, 18, 6))
    out.append(Case('pad limit', 9, 15, 'REFLECT', 'linear', 60, 8, 18, 6))
    for (kh, kw), mode, act in (((7, 3), 'CONSTANT', 'leaky_relu'), ((9, 15), 'SYMMETRIC', 'tanh'), ((4, 13), 'REFLECT', 'linear')):
        for Cin, Cout in ((3, 4), (12, 20), (28, 24), (64, 32), (32, 64), (17, 33)):
            H, W = _size(kh, kw)[:2]
            out.append(Case('channels', kh, kw, mode, act, H, W, Cin, Cout))
    out.append(Case('slices', 3, 7, 'CONSTANT', 'leaky_relu', 40, 45, 6, 5, slices=True))
    out.append(Case('slices', 15, 9, 'SYMMETRIC', 'tanh', 60, 62, 18, 6, slices=True))
    return out


CASES = _cases()
POST_DONE = set()      # tile sizes whose fused backward has run with a Post


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device='cuda')


def nhwc(a):
    return dev(np.asarray(a).transpose(0, 2, 3, 1))


def nchw(t):
    return t.detach().cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


CANARY = 7.5


def sliced(a_nchw, offset, width=48):
    """The tensor as a channel slice at `offset` of a (N, H, W, width) buffer filled with the canary value; returns (view, buffer)."""
    t = nhwc(a_nchw)
    buf = torch.full(t.shape[:3] + (width,), CANARY, dtype=torch.float32, device='cuda')
    view = buf[..., offset:offset + t.shape[3]]
    view.copy_(t)
    return view, buf


def canary_intact(buf, offset, C):
    return bool((buf[..., :offset] == CANARY).all()) and bool((buf[..., offset + C:] == CANARY).all())


def act_prime(a, act):
    if act == 'leaky_relu':
        return np.where(a > 0, 1.0, np_ops.LEAKY_ALPHA)
    return 1.0 - a * a if act == 'tanh' else np.ones_like(a)


class Problem:
    """One case's data, fp64 references and device tensors (computed once, shared by the routes)."""

    def __init__(self, c):
        from poisson_cnn_amd import ops
        self.c = c
        rng = np.random.default_rng([c.kh, c.kw, c.Cin, c.Cout, c.H, c.W, c.pt, c.pl])
        N = 2
        self.x = f32(rng.standard_normal((N, c.Cin, c.H, c.W)))
        self.w = f32(rng.standard_normal((c.kh, c.kw, c.Cin, c.Cout)) / np.sqrt(c.kh * c.kw * c.Cin))
        self.b = f32(rng.standard_normal(c.Cout))
        self.dz = f32(rng.standard_normal((N, c.Cout, c.Ho, c.Wo)))
        self.value = PAD_VALUE if c.mode == 'CONSTANT' else 0.0
        geo = (c.pt, c.pl, (c.Ho, c.Wo), c.mode)
        self.pre = G.ref_conv(self.x, self.w, self.b, *geo, self.value, 'linear')
        self.a = np_ops.activation(self.pre, c.act)
        self.y = self.a
        if c.slices:
            self.sc, self.sh = f32(rng.uniform(0.5, 1.5, c.Cout)), f32(rng.standard_normal(c.Cout))
            self.res = f32(rng.standard_normal(self.a.shape))
            self.y = self.a * self.sc[None, :, None, None] + self.sh[None, :, None, None] + self.res
        # gradients of the linear layer with zero padding value (the fused backward takes CONSTANT padding with value 0 only)
        self.dx, self.dw, _ = G.gradients(self.x, self.w, None, self.dz, c.pt, c.pl, c.mode, 0.0)
        # element-wise bounds of the direct route: the same sums over absolute values
        self.abs_pre = G.ref_conv(np.abs(self.x), np.abs(self.w), np.abs(self.b), *geo, abs(self.value), 'linear') if c.act == 'linear' else None
        self.abs_dx, self.abs_dw, _ = G.gradients(np.abs(self.x), np.abs(self.w), None, np.abs(self.dz), c.pt, c.pl, c.mode, 0.0)
        # the skip connection / producer of the fused backward
        self.skip = f32(rng.standard_normal(self.x.shape))
        self.prod_a = f32(np.tanh(rng.standard_normal(self.x.shape)))
        if c.slices:
            self.xd, self.xbuf = sliced(self.x, 3)
        else:
            self.xd = nhwc(self.x)
        self.wd, self.bd, self.dzd = dev(self.w), dev(self.b), nhwc(self.dz)
        self.wf = ops.flip_transpose_weights(self.wd)
        assert np.array_equal(self.wf.cpu().numpy(), self.w[::-1, ::-1].transpose(0, 1, 3, 2).astype(np.float32))

    def forward(self):
        """-> (y, act_out or None), checking the canaries of the slice rows"""
        from poisson_cnn_amd import ops
        c = self.c
        kw = dict(pad_top=c.pt, pad_left=c.pl, out_hw=(c.Ho, c.Wo), pad_mode=c.mode, pad_value=self.value, act=c.act)
        if not c.slices:
            return nchw(ops.conv2d_fwd(self.xd, self.wd, self.bd, **kw)), None
        out, obuf = sliced(np.zeros_like(self.y), 30)
        res, rbuf = sliced(self.res, 3)
        aout, abuf = sliced(np.zeros_like(self.y), 30)
        ops.conv2d_fwd(self.xd, self.wd, self.bd, bn_scale=dev(self.sc), bn_shift=dev(self.sh), residual=res, out=out, act_out=aout, **kw)
        assert canary_intact(obuf, 30, c.Cout) and canary_intact(abuf, 30, c.Cout) and canary_intact(rbuf, 3, c.Cout) and canary_intact(self.xbuf, 3, c.Cin)
        assert np.array_equal(nchw(res), self.res) and np.array_equal(nchw(self.xd), self.x)
        return nchw(out), nchw(aout)

    def dgrad(self):
        from poisson_cnn_amd import ops
        c = self.c
        if c.mode == 'CONSTANT':
            return nchw(ops.conv2d_fwd(self.dzd, self.wf, None, pad_top=c.kh - 1 - c.pt, pad_left=c.kw - 1 - c.pl, out_hw=(c.H, c.W)))
        gp = ops.conv2d_fwd(self.dzd, self.wf, None, pad_top=c.kh - 1, pad_left=c.kw - 1, out_hw=(c.Ho + c.kh - 1, c.Wo + c.kw - 1))
        return nchw(ops.pad_fold_bwd(gp, (c.H, c.W), ((c.pt, c.pb), (c.pl, c.pr)), c.mode))

    def wgrad(self):
        from poisson_cnn_amd import ops
        c = self.c
        a, b = (ops.conv2d_wgrad(self.xd, self.dzd, self.w.shape, pad_top=c.pt, pad_left=c.pl, pad_mode=c.mode, pad_value=0.0).clone() for _ in range(2))
        assert torch.equal(a, b), 'weight gradient not repeatable'
        return a.cpu().numpy().astype(np.float64)

    def fused(self, post=False):
        """-> None (declined) or dict(dx, dw[, raw, dbias])"""
        from poisson_cnn_amd import ops
        c = self.c
        res = nhwc(self.skip) if c.mode == 'CONSTANT' else None
        outs = []
        for _ in range(2):
            dw = torch.full(self.w.shape, CANARY, dtype=torch.float32, device='cuda')
            p = ops.Post(nhwc(self.prod_a), 'tanh', torch.full((c.Cin,), CANARY, device='cuda'), want_raw=True) if post else None
            out = ops.conv2d_bwd_fused(self.xd, self.dzd, self.w.shape, self.wf, pad_top=c.pt, pad_left=c.pl, pad_mode=c.mode, dw=dw,
                                       residual=res.clone() if res is not None else None, post=p)
            if out is None:
                return None
            assert not post or p.applied
            outs.append((out.clone(), dw, p.raw.clone() if post else None, p.dbias.clone() if post else None))
        for u, v in zip(*outs):
            assert u is None or torch.equal(u, v), 'fused backward not repeatable'
        out, dw, raw, dbias = outs[0]
        r = {'dw': dw.cpu().numpy().astype(np.float64)}
        if c.mode == 'CONSTANT':
            r['dx'] = nchw(out)
        else:
            r['dx'] = nchw(ops.pad_fold_bwd(out, (c.H, c.W), ((c.pt, c.pb), (c.pl, c.pr)), c.mode))
        if post:
            r['raw'], r['dbias'] = nchw(raw), dbias.cpu().numpy().astype(np.float64)
        return r


def check(route, op, got, ref, kh, kw, bound, tag):
    """Whole-tensor bound on every route, the bound per region on the spectral routes."""
    e = G.rel(got, ref)
    figure(route, op, e, bound)
    print('%-12s %-6s whole %.3e (bound %.0e)  %s' % (route, op, e, bound, tag))
    assert e <= bound, '%s %s %s: whole tensor rel-L2 %.3e > %.0e' % (tag, route, op, e, bound)
    if route in SPECTRAL and got.ndim == 4:
        if 'dw' in op or op == 'wgrad':                      # a filter gradient (kh, kw, Cin, Cout): its regions are the output channels
            got, ref = (a.transpose(3, 0, 1, 2).reshape(1, a.shape[3], a.shape[0], -1) for a in (got, ref))
            kh = kw = 1
        name, e = G.worst_region(got, ref, kh, kw)
        b = REGION_BOUNDS.get((name.split()[0], op), bound)
        figure(route, op + ' region', e, b)
        print('%-12s %-6s worst region %s %.3e' % (route, op, name, e))
        assert e <= b, '%s %s %s: region %s rel-L2 %.3e > %.0e' % (tag, route, op, name, e, b)


def elementwise(op, got, ref, abs_ref, K, tag):
    bound = G.gamma(K) * abs_ref
    worst = float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)))
    figure('direct', op + ' elementwise', worst, 1.0)
    print('direct       %-6s element-wise |err| / (gamma(%d) sum|products|) max %.3f  %s' % (op, K, worst, tag))
    assert worst <= 1.0, '%s direct %s: element-wise error %.3f x gamma(%d) x sum |products|' % (tag, op, worst, K)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_case_on_every_route(c):
    P = Problem(c)
    N = 2
    got = {}
    for route in ROUTES:
        with selected(route):
            r = got[route] = {}
            if route.startswith('spec64') and not c.can64:
                # pick_tile keeps 32-point tiles below 9 taps whatever is forced: the same kernel, the same bits
                y, _ = P.forward()
                assert same(y, got[FALLBACK[route]]['fwd']), '%s: tile 64 forced on a %dx%d filter must run the 32-point kernels' % (c.id, c.kh, c.kw)
                BELOW64.setdefault(route, []).append(c.id)
                continue
            r['fwd'], r['act_out'] = P.forward()
            r['dgrad'] = P.dgrad()
            r['wgrad'] = P.wgrad()
            if route in SPECTRAL:
                r['fused'] = P.fused()
                T = 64 if route.startswith('spec64') else 32
                if r['fused'] is not None and c.mode == 'CONSTANT' and c.Cin <= 32 and (T, route) not in POST_DONE and c.kind != 'channels':
                    r['post'] = P.fused(post=True)
                    assert r['post'] is not None
                    POST_DONE.add((T, route))
            torch.cuda.synchronize()
        for op, ref, bound in (('fwd', P.y, TOL), ('dgrad', P.dx, TOL), ('wgrad', P.dw, TOL_RED)):
            fb = FALLBACK.get(route)
            declined = fb is not None and same(r[op], got[fb][op])
            note(c.kind, route, op, declined)
            if declined:
                print('%-12s %-6s declined (bit-identical to %s)  %s' % (route, op, fb, c.id))
                continue
            check(route, op, r[op], ref, c.kh, c.kw, bound, c.id)
            if op == 'fwd' and r['act_out'] is not None:
                check(route, 'fwd', r['act_out'], P.a, c.kh, c.kw, bound, c.id + ' act_out')
            nb = NEIGHBOUR.get(route)
            if nb is not None and op in got[nb]:
                d = G.rel(r[op], got[nb][op])
                assert 0 < d < bound, '%s %s %s: differs from %s by %.3e' % (c.id, route, op, nb, d)
        if route == 'direct':
            if c.act == 'linear' and not c.slices:
                elementwise('fwd', r['fwd'], P.pre, P.abs_pre, c.kh * c.kw * c.Cin + 1, c.id)
            elementwise('dgrad', r['dgrad'], P.dx, P.abs_dx, c.kh * c.kw * c.Cout + (0 if c.mode == 'CONSTANT' else 3), c.id)
            elementwise('wgrad', r['wgrad'], P.dw, P.abs_dw, N * c.Ho * c.Wo, c.id)
        if route in SPECTRAL:
            f = r['fused']
            fb = got[FALLBACK[route]].get('fused')
            declined = f is None or (fb is not None and same(f['dx'], fb['dx']) and same(f['dw'], fb['dw']))      # (64-point tiles forced on packed tiles: the 32-point kernels)
            note(c.kind, route, 'fused', declined)
            if declined:
                print('%-12s fused  declined  %s' % (route, c.id))
                assert f is not None or c.Cout > 32, c.id  # pcnn_conv2d_bwd_spectral_eligible with the route forced: only Cout > 32 (Cin <= 64 here)
            else:
                skip = P.skip if c.mode == 'CONSTANT' else 0.0
                check(route, 'fused dx', f['dx'] - skip, P.dx, c.kh, c.kw, TOL, c.id)
                check(route, 'fused dw', f['dw'], P.dw, c.kh, c.kw, TOL_RED, c.id)
                nb = NEIGHBOUR[route]
                if nb in SPECTRAL and got[nb].get('fused') is not None:
                    d = G.rel(f['dx'], got[nb]['fused']['dx'])
                    assert 0 < d < TOL, '%s %s fused: differs from %s by %.3e' % (c.id, route, nb, d)
            if 'post' in r:
                p = r['post']
                raw = P.dx + P.skip
                dxa = raw * act_prime(P.prod_a, 'tanh')
                check(route, 'post raw', p['raw'], raw, c.kh, c.kw, TOL, c.id)
                check(route, 'post dx', p['dx'], dxa, c.kh, c.kw, TOL, c.id)
                check(route, 'post dw', p['dw'], P.dw, c.kh, c.kw, TOL_RED, c.id)
                check(route, 'post db', p['dbias'], dxa.sum(axis=(0, 2, 3)), c.kh, c.kw, TOL_RED, c.id)
                note('post', route, 'post', False)


@pytest.mark.parametrize('route', ROUTES)
def test_one_step_beyond_the_tf_pad_limit_is_refused_and_nothing_is_written(route):
    """SYMMETRIC with size = k // 2 - 1 and REFLECT with size = k // 2, in y and in x: pcnn_conv2d_fwd refuses on the host (nothing is launched),
    the output buffer keeps its contents, and the handle stays usable."""
    from poisson_cnn_amd import ops
    for (kh, kw), mode, H, W in (((15, 9), 'SYMMETRIC', 6, 62), ((15, 9), 'REFLECT', 7, 62), ((9, 15), 'SYMMETRIC', 60, 6), ((9, 15), 'REFLECT', 60, 7)):
        x = torch.randn(2, H, W, 18, device='cuda')
        w = torch.randn(kh, kw, 18, 6, device='cuda')
        out = torch.full((2, H, W, 6), CANARY, device='cuda')
        with selected(route):
            with pytest.raises(RuntimeError, match='padding exceeds'):
                ops.conv2d_fwd(x, w, None, pad_top=kh // 2, pad_left=kw // 2, pad_mode=mode, out=out)
            torch.cuda.synchronize()
            assert bool((out == CANARY).all())
            y = ops.conv2d_fwd(x, w, None, pad_top=kh // 2, pad_left=kw // 2, pad_mode='CONSTANT', out=out)
        assert torch.isfinite(y).all() and not bool((out == CANARY).any())


# ------------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize('route', ROUTES)
def test_the_comparison_rejects_wrong_but_valid_problems(route):
    """The proof that the sweep would notice, through valid launches only: each route is handed a legitimately different problem and the
    comparison must reject it.  (a) the filter with its two tap axes transposed, (b) pad_top and pad_left exchanged, (c) the weight gradient
    against the reference's taps transposed - all three must miss the whole-tensor bound; (d) the kernel's own correct result with one of 32
    output channels scaled by 1 + 8e-6 on the host: built to pass the whole-tensor bound (8e-6 / sqrt(32) = 1.4e-6) and to miss the
    per-channel one."""
    from poisson_cnn_amd import ops
    rng = np.random.default_rng(77)
    N, H, W, Cin, Cout, kh, kw = 2, 60, 62, 18, 32, 9, 11
    x = f32(rng.standard_normal((N, Cin, H, W)))
    w = f32(rng.standard_normal((kh, kw, Cin, Cout)) / np.sqrt(kh * kw * Cin))
    b = f32(rng.standard_normal(Cout))
    ref = G.ref_conv(x, w, b, kh // 2, kw // 2, (H, W))
    xd, wd, bd = nhwc(x), dev(w), dev(b)
    with selected(route):
        good = nchw(ops.conv2d_fwd(xd, wd, bd, pad_top=kh // 2, pad_left=kw // 2))
        wT = wd.permute(1, 0, 2, 3).contiguous()
        a = nchw(ops.conv2d_fwd(xd, wT, bd, pad_top=kw // 2, pad_left=kh // 2))
        bb = nchw(ops.conv2d_fwd(xd, wd, bd, pad_top=kw // 2, pad_left=kh // 2, out_hw=(H + 1, W - 1)))
        ws = f32(rng.standard_normal((9, 9, Cin, Cout)))
        dz = f32(rng.standard_normal((N, Cout, H, W)))
        dw = ops.conv2d_wgrad(xd, nhwc(dz), ws.shape, pad_top=4, pad_left=4).cpu().numpy().astype(np.float64)
    assert G.rel(good, ref) <= TOL
    assert a.shape == ref.shape and G.rel(a, ref) > TOL, 'transposed taps not noticed'
    # exchanged offsets: the valid descriptor with pad_top = 5, pad_left = 4 has its output one row longer and one column shorter; on the common window
    assert G.rel(bb[:, :, :H, :W - 1], ref[:, :, :, :W - 1]) > TOL, 'exchanged offsets not noticed'
    assert G.rel(bb, G.ref_conv(x, w, b, kw // 2, kh // 2, (H + 1, W - 1))) <= TOL
    _, dw_ref, _ = G.gradients(x, ws, None, dz, 4, 4)
    assert G.rel(dw, dw_ref) <= TOL_RED
    assert G.rel(dw, dw_ref.transpose(1, 0, 2, 3)) > TOL_RED, 'transposed weight-gradient taps not noticed'
    bad = good.copy()
    bad[:, 13] *= 1 + 8e-6
    whole, (name, worst) = G.rel(bad, ref), G.worst_region(bad, ref, kh, kw)
    print('%s: correct result %.3e, one channel scaled: whole %.3e, worst region %s %.3e' % (route, G.rel(good, ref), whole, name, worst))
    assert G.worst_region(good, ref, kh, kw)[1] <= TOL
    assert worst > TOL and name == 'channel 13', 'the per-channel bound does not notice a defect confined to one channel'
    assert whole <= TOL, 'the kernel\'s own error leaves no room under the whole-tensor bound: %.3e' % whole


# ------------------------------------------------------------------------------------------------------------------ the Python side
@pytest.mark.parametrize('kh,kw,mode', [(3, 7, 'SYMMETRIC'), (15, 9, 'REFLECT'), (15, 9, 'CONSTANT')])
@pytest.mark.parametrize('route', ['direct', 'spec32-fft', 'spec64-fft'])
def test_conv_unit_with_a_rectangular_kernel_through_autograd(kh, kw, mode, route):
    """layers.ConvUnit((kh, kw)) (built by keras_layers.Conv2D under apply_advanced_padding_and_call_conv_layer) on the torch.autograd tape:
    its pads_y / pads_x, the padded-domain fold and the fused backward see the two axes apart."""
    from poisson_cnn_amd import keras_layers as K
    from poisson_cnn_amd.autograd import Differentiable
    rng = np.random.default_rng(kh)
    N, Cin, Cout, H, W = 2, 18, 6, 60, 62
    x = f32(rng.standard_normal((N, Cin, H, W)))
    dy = f32(rng.standard_normal((N, Cout, H, W)))
    with selected(route):
        conv = K.Conv2D(Cout, (kh, kw), activation='tanh', seed=kh)
        mod = Differentiable(K.apply_advanced_padding_and_call_conv_layer(mode, conv, constant_padding_value=PAD_VALUE if mode == 'CONSTANT' else 0.0))
        xt = torch.tensor(x, dtype=torch.float32, device='cuda', requires_grad=True)
        with torch.no_grad():
            mod(xt)                                         # builds the layer
        wts = {n: f32(t if n.endswith('kernel') else rng.standard_normal(t.shape) * 0.2) for n, t in zip(conv.weight_names, conv.get_weights())}
        conv.set_weights(wts)
        y = mod(xt)
        y.backward(torch.tensor(dy, dtype=torch.float32, device='cuda'))
        grads = {n: g.detach().cpu().numpy().astype(np.float64) for n, g in conv.gradients.items()}
    assert conv.unit.pads_y == np_ops.advanced_pad_amounts(kh) and conv.unit.pads_x == np_ops.advanced_pad_amounts(kw)
    wk, bk = wts['conv/kernel'], wts['conv/bias']
    assert wk.shape == (kh, kw, Cin, Cout)
    value = PAD_VALUE if mode == 'CONSTANT' else 0.0
    ref = G.ref_conv(x, wk, bk, kh // 2, kw // 2, (H, W), mode, value, 'tanh')
    dx, dw, db = G.gradients(x, wk, bk, dy, kh // 2, kw // 2, mode, value, 'tanh')
    got = y.detach().cpu().numpy().astype(np.float64)
    for name, g, r, bound in (('y', got, ref, TOL), ('dx', xt.grad.cpu().numpy().astype(np.float64), dx, TOL), ('dw', grads['conv/kernel'], dw, TOL_RED),
                              ('db', grads['conv/bias'], db, TOL_RED)):
        e = G.rel(g, r)
        print('ConvUnit (%d, %d) %s %s: %s %.3e' % (kh, kw, mode, route, name, e))
        assert e <= bound, (name, e)


@pytest.mark.parametrize('route', ['direct', 'spec32-fft', 'spec64-fft'])
def test_keras_conv2d_same_padding_with_a_rectangular_kernel(route):
    """keras_layers.Conv2D(kernel_size=(9, 15), padding='same'): Keras' SAME pads per axis, forward and backward."""
    from poisson_cnn_amd import keras_layers as K
    rng = np.random.default_rng(3)
    N, Cin, Cout, H, W = 2, 18, 6, 60, 62
    x = f32(rng.standard_normal((N, Cin, H, W)))
    dy = f32(rng.standard_normal((N, Cout, H, W)))
    with selected(route):
        conv = K.Conv2D(Cout, kernel_size=(9, 15), padding='same', activation='tf.nn.leaky_relu', seed=1)
        conv(x)
        wts = {n: f32(t if n.endswith('kernel') else rng.standard_normal(t.shape) * 0.2) for n, t in zip(conv.weight_names, conv.get_weights())}
        conv.set_weights(wts)
        y = conv(x, training=True)
        dxg = conv.backward(dy)
        grads = {n: g.detach().cpu().numpy().astype(np.float64) for n, g in conv.gradients.items()}
    wk, bk = wts['conv/kernel'], wts['conv/bias']
    ref = G.ref_conv(x, wk, bk, 4, 7, (H, W), 'CONSTANT', 0.0, 'leaky_relu')
    assert np.abs(ref - np_ops.same_conv2d(x, wk, bk, 'leaky_relu')).max() <= 1e-12
    dx, dw, db = G.gradients(x, wk, bk, dy, 4, 7, 'CONSTANT', 0.0, 'leaky_relu')
    as64 = lambda t: t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    for name, g, r, bound in (('y', as64(y), ref, TOL), ('dx', as64(dxg), dx, TOL), ('dw', grads['conv/kernel'], dw, TOL_RED), ('db', grads['conv/bias'], db, TOL_RED)):
        e = G.rel(g, r)
        print('Conv2D (9, 15) same %s: %s %.3e' % (route, name, e))
        assert e <= bound, (name, e)
    with pytest.raises(NotImplementedError):
        K.Conv2D(Cout, kernel_size=(9, 15), padding='valid')(x, training=True)


# ------------------------------------------------------------------------------------------------------------------ per-sample filters
@pytest.mark.parametrize('kh,kw,mode', [(3, 7, 'CONSTANT'), (7, 3, 'SYMMETRIC'), (4, 13, 'REFLECT')])
@pytest.mark.parametrize('route', ['mfma', 'valu'])
def test_grouped_kernels_with_rectangular_filters(kh, kw, mode, route):
    """grouped_conv2d_fwd, its flip_transpose data gradient and grouped_conv2d_wgrad with kh != kw on the matrix-core and the vector-ALU route."""
    from poisson_cnn_amd import ops
    rng = np.random.default_rng(kh * 10 + kw)
    N, Cin, Cout, H, W = 3, 3, 4, 37, 50
    wshape, nk = (kh, kw, Cin, Cout), kh * kw * Cin * Cout
    x = f32(rng.standard_normal((N, Cin, H, W)))
    kb = f32(rng.standard_normal((N, nk + Cout)) / np.sqrt(kh * kw * Cin))
    dz = f32(rng.standard_normal((N, Cout, H, W)))
    (pt, pb), (pl, pr) = np_ops.advanced_pad_amounts(kh), np_ops.advanced_pad_amounts(kw)
    if route == 'valu':
        os.environ['PCNN_GROUPED_VALU'] = '1'
    try:
        for what in ('fwd', 'wgrad'):
            assert ops.grouped_uses_mfma((N, H, W, Cin), wshape, (H, W), what) == (route == 'mfma'), what
        xd, kd, dzd = nhwc(x), dev(kb), nhwc(dz)
        y = ops.grouped_conv2d_fwd(xd, kd, wshape, kd[:, nk:], pad_top=pt, pad_left=pl, out_hw=(H, W), pad_mode=mode, pad_value=PAD_VALUE, act='tanh')
        dk = [torch.zeros_like(kd) for _ in range(2)]
        for d in dk:
            ops.grouped_conv2d_wgrad(xd, dzd, wshape, d, pad_top=pt, pad_left=pl, pad_mode=mode, pad_value=0.0)
        assert torch.equal(dk[0], dk[1])
        gp = ops.grouped_conv2d_fwd(dzd, kd, wshape, None, pad_top=kh - 1, pad_left=kw - 1, out_hw=(H + kh - 1, W + kw - 1), flip_transpose=True)
        dxg = nchw(ops.pad_fold_bwd(gp, (H, W), ((pt, pb), (pl, pr)), mode))
        y, dwg = nchw(y), dk[0].cpu().numpy().astype(np.float64)
    finally:
        os.environ.pop('PCNN_GROUPED_VALU', None)
    for n in range(N):
        wn, bn = kb[n, :nk].reshape(wshape), kb[n, nk:]
        ref = G.ref_conv(x[n:n + 1], wn, bn, pt, pl, (H, W), mode, PAD_VALUE, 'tanh')
        dx, dw, _ = G.gradients(x[n:n + 1], wn, None, dz[n:n + 1], pt, pl, mode, 0.0)
        for name, g, r, bound in (('y', y[n:n + 1], ref, TOL), ('dx', dxg[n:n + 1], dx, TOL), ('dw', dwg[n, :nk].reshape(wshape), dw, TOL_RED)):
            e = G.rel(g, r)
            print('grouped (%d, %d) %s %s sample %d: %s %.3e' % (kh, kw, mode, route, n, name, e))
            assert e <= bound, (name, n, e)
        assert np.all(dwg[n, nk:] == 0)


# ------------------------------------------------------------------------------------------------------------------ the ledger
def test_every_cell_of_the_table_ran_and_the_decline_cap_holds():
    """Runs last: every (case kind, route, operation) cell has at least one case that the route really took, no (route, operation) declined
    more than a quarter of its cases, the Post form ran once per spectral route, and the cases below the 64-point tiles' filter size are
    exactly the ones the table says."""
    assert LEDGER, 'run the whole module: this test reads what test_case_on_every_route recorded'
    ops_of = lambda route: ('fwd', 'dgrad', 'wgrad') + (('fused',) if route in SPECTRAL else ())
    lines, bad = [], []
    for route in ROUTES:
        for op in ops_of(route):
            ran = sum(LEDGER.get((k, route, op), [0, 0])[0] for k in KINDS)
            dec = sum(LEDGER.get((k, route, op), [0, 0])[1] for k in KINDS)
            empty = [k for k in KINDS if LEDGER.get((k, route, op), [0, 0])[0] == 0]
            lines.append('%-12s %-6s ran %3d declined %2d  empty cells: %s' % (route, op, ran, dec, empty or 'none'))
            if empty or 4 * dec > ran + dec:
                bad.append(lines[-1])
        if route in SPECTRAL:
            assert LEDGER.get(('post', route, 'post'), [0, 0])[0] >= 1, route + ': no fused backward with a Post'
    print('\n'.join(lines))
    print('below64: %s' % {r: len(v) for r, v in BELOW64.items()})
    for (route, op), v in sorted(FIGURES.items()):
        print('worst figure / bound  %-12s %-18s %.3f' % (route, op, v))
    assert not bad, '\n'.join(bad)
    below = sorted(c.id for c in CASES if not c.can64)
    for route in ('spec64-mfma', 'spec64-fft'):
        assert sorted(BELOW64.get(route, [])) == below
