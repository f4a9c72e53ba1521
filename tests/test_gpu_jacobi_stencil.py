"""The Jacobi smoother for any cross-shaped FD stencil on the temporally blocked kernels of csrc/stencil.hip, and the physics-informed loss with
rectangular stencils, against the fp64 oracle (oracle/np_ops.py jacobi_iterations, oracle/torch_twin.py for the adjoint, oracle/loss.py).

Bounds.  One sweep: the project's per-op 2e-6 rel-L2.  More than one sweep: Jacobi on the operators of 5 points and more amplifies the checkerboard
mode (the 5-point fourth-order line: |lambda| = 17/15 per sweep), so rounding errors grow with the sweep count and a fixed bound means nothing.  The
same recurrence is therefore evaluated in float32 numpy on the CPU (`recurrence(..., np.float32)`: the layer's own float32 coefficient rows, the taps
summed in the kernel's order but without fused multiply-adds), its rel-L2 against the fp64 oracle is taken for that very case, and the GPU result
must stay within 4x that figure, floored at 2e-6; the 4 allows for a different but fixed summation order.  The adjoint follows the same rule."""
import functools

import numpy as np
import pytest
import torch

from oracle import np_ops, torch_twin, loss as oloss

pytestmark = pytest.mark.gpu
TOL = 2e-6

STENCILS = [((3, 3), (2, 2)), ((5, 5), (2, 2)), ((3, 7), (2, 2)), ((7, 3), (2, 2)), ((9, 9), (2, 2)), ((5, 7), (4, 2))]
N = 3


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda')


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def nhw1(a):                       # (N,1,H,W) numpy -> the kernels' (N,H,W,1)
    return dev(np.asarray(a)[:, 0, :, :, None])


def back(t):                       # (N,H,W,1) device -> (N,1,H,W) numpy float64
    return t.detach().cpu().numpy()[:, None, :, :, 0].astype(np.float64)


def limits(ss):
    from poisson_cnn_amd import ops
    return ops.jacobi_tile(), ops.jacobi_k_max(*ss)


def shapes(ss):
    T, _ = limits(ss)
    ry, rx = ss[0] // 2, ss[1] // 2
    return [(11, 13), (2 * ry + 1, 13), (11, 2 * rx + 1), (2 * T + 1, 3 * T + 1)]


def sweep_counts(ss):
    _, k = limits(ss)
    return [1, k, k + 1, 2 * k + 3]


@functools.lru_cache(maxsize=None)
def inputs(H, W):
    rng = np.random.default_rng(1000 * H + W)
    u = f32(rng.standard_normal((N, 1, H, W)))
    rhs = f32(rng.standard_normal((N, 1, H, W)))
    dx = f32(rng.uniform(5e-3, 5e-2, (N, 2)))                     # the reference's range, a distinct anisotropic row per sample
    dout = f32(rng.standard_normal((N, 1, H, W)))
    return u, rhs, dx, dout                                        # shared by every test of that shape: read, never written


def rows_of(ss, od, dx, dtype):
    """The kernel's coefficient rows: float32 as the layer builds them (on CPU tensors), or float64 from the oracle's composition."""
    if dtype == np.float32:
        from poisson_cnn_amd.layers import JacobiIterationLayer
        return JacobiIterationLayer(1, ss, od).coefficient_rows(torch.from_numpy(dx.astype(np.float32))).numpy()
    coeff = np_ops.build_fd_coefficients(list(ss), list(od), 2)
    c = (ss[0] // 2, ss[1] // 2)
    diag = coeff[(Ellipsis,) + c].copy()
    lu = coeff.copy()
    lu[(Ellipsis,) + c] = 0.0
    dxp = (1.0 / dx) ** np.array(od, dtype=np.float64)
    kern = np.einsum('dij,bd->bij', lu, dxp)
    return np.concatenate([kern[:, :, c[1]], kern[:, c[0], :], (1.0 / (dxp @ diag))[:, None]], axis=1)


def recurrence(x, rhs, rows, ss, n, dtype, adjoint=False, ring=None):
    """n sweeps (or n adjoint sweeps) in `dtype` numpy.  rows (N, sy+sx+1) as the kernel takes them.  ring: the frozen border's widths, (sy//2, sx//2)
    unless a deliberately wrong twin narrows it (values past the image edge then read as zero)."""
    sy, sx = ss
    ry, rx = sy // 2, sx // 2
    py, px = (ry, rx) if ring is None else ring
    x = np.asarray(x, dtype=dtype)[:, 0]
    rhs = np.asarray(rhs, dtype=dtype)[:, 0]
    rows = np.asarray(rows, dtype=dtype)
    Nn, H, W = x.shape
    mask = np.zeros((H, W), dtype=dtype)
    mask[py:H - py, px:W - px] = 1
    dinv = rows[:, sy + sx][:, None, None]
    for _ in range(n):
        src = x * mask if adjoint else x                       # the adjoint gathers from interior points only
        p = np.zeros((Nn, H + 2 * ry, W + 2 * rx), dtype=dtype)
        p[:, ry:ry + H, rx:rx + W] = src
        acc = np.zeros_like(x)
        for i in range(sy):
            if i != ry:
                o = (i - ry) * (-1 if adjoint else 1)
                acc = acc + rows[:, i][:, None, None] * p[:, ry + o:ry + o + H, rx:rx + W]
        for j in range(sx):
            if j != rx:
                o = (j - rx) * (-1 if adjoint else 1)
                acc = acc + rows[:, sy + j][:, None, None] * p[:, ry:ry + H, rx + o:rx + o + W]
        if adjoint:
            x = (x * (1 - mask) - dinv * acc).astype(dtype)
        else:
            x = (mask * (dinv * (rhs - acc)) + (1 - mask) * x).astype(dtype)
    return x[:, None].astype(np.float64)


@functools.lru_cache(maxsize=None)
def references(ss, od, H, W):
    """Per sweep count: the fp64 oracle's forward, the oracle twin's adjoint (autograd), and the float32-CPU recurrence's error against each."""
    u, rhs, dx, dout = inputs(H, W)
    counts = sweep_counts(ss)
    r32 = rows_of(ss, od, dx, np.float32)
    out = {}
    x = u
    done = 0
    for n in counts:
        for _ in range(n - done):                               # n sweeps of the oracle == n calls of one sweep (fp64, the same operations)
            x = np_ops.jacobi_iterations(x, rhs, dx, 1, ss, od)
        done = n
        ut = torch.tensor(u, requires_grad=True)
        (torch_twin.jacobi_iterations(ut, rhs, dx, n, ss, od) * torch.tensor(dout)).sum().backward()
        e_f = rel(recurrence(u, rhs, r32, ss, n, np.float32), x)
        e_b = rel(recurrence(dout, rhs, r32, ss, n, np.float32, adjoint=True), ut.grad.numpy())
        out[n] = (x, ut.grad.numpy().copy(), e_f, e_b)
    return out


def bound(n, e_cpu32):
    return TOL if n == 1 else max(TOL, 4.0 * e_cpu32)


def gpu_fwd(ss, od, H, W, n):
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    u, rhs, dx, _ = inputs(H, W)
    coef = JacobiIterationLayer(n, ss, od).coefficient_rows(dev(dx))
    return back(ops.jacobi_fused(nhw1(u), nhw1(rhs), coef, ss, n))


def gpu_bwd(ss, od, H, W, n):
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    _, _, dx, dout = inputs(H, W)
    coef = JacobiIterationLayer(n, ss, od).coefficient_rows(dev(dx))
    return back(ops.jacobi_fused_bwd(nhw1(dout), coef, ss, n))


@pytest.mark.parametrize('ss,od', STENCILS)
def test_forward_and_adjoint_against_the_oracle(ss, od):
    """(a) and (c): every shape x every sweep count.  Prints each figure before asserting it (DESIGN.md section 11 quotes them)."""
    fails = []
    for (H, W) in shapes(ss):
        ref = references(ss, od, H, W)
        for n in sweep_counts(ss):
            xf, xb, e_f, e_b = ref[n]
            g_f, g_b = rel(gpu_fwd(ss, od, H, W, n), xf), rel(gpu_bwd(ss, od, H, W, n), xb)
            print('jacobi %s/%s %dx%d n=%d: fwd gpu %.2e cpu32 %.2e bound %.2e | bwd gpu %.2e cpu32 %.2e bound %.2e'
                  % (list(ss), list(od), H, W, n, g_f, e_f, bound(n, e_f), g_b, e_b, bound(n, e_b)))
            if not g_f < bound(n, e_f):
                fails.append(('fwd', H, W, n, g_f, bound(n, e_f)))
            if not g_b < bound(n, e_b):
                fails.append(('bwd', H, W, n, g_b, bound(n, e_b)))
    assert not fails, fails


@pytest.mark.parametrize('ss,od', STENCILS)
def test_fusing_is_exact(ss, od):
    """(b) n sweeps in as few launches as possible == n launches of one sweep each, bit for bit, forward and adjoint, on the multi-tile shape and
    the small one: a halo one point short, a ring that thaws inside a halo or an rhs halo off by one all show here."""
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    for (H, W) in (shapes(ss)[3], shapes(ss)[0]):
        u, rhs, dx, dout = inputs(H, W)
        coef = JacobiIterationLayer(1, ss, od).coefficient_rows(dev(dx))
        ud, rd, dd = nhw1(u), nhw1(rhs), nhw1(dout)
        for n in sweep_counts(ss)[1:]:
            a, b = ud, dd
            for _ in range(n):
                a = ops.jacobi_fused(a, rd, coef, ss, 1)
                b = ops.jacobi_fused_bwd(b, coef, ss, 1)
            assert torch.equal(ops.jacobi_fused(ud, rd, coef, ss, n), a), (H, W, n)
            assert torch.equal(ops.jacobi_fused_bwd(dd, coef, ss, n), b), (H, W, n)


@pytest.mark.parametrize('ss,od', [((3, 3), (2, 2)), ((5, 7), (4, 2)), ((9, 9), (2, 2))])
def test_adjoint_identity(ss, od):
    """<J v, w> == <v, J^T w> with J v the forward at rhs = 0; fp32 device results, the inner products in fp64 on the host, 1e-5 relative."""
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    H, W = shapes(ss)[3]
    v, _, dx, w = inputs(H, W)
    coef = JacobiIterationLayer(1, ss, od).coefficient_rows(dev(dx))
    for n in (1, sweep_counts(ss)[2]):
        Jv = back(ops.jacobi_fused(nhw1(v), torch.zeros_like(nhw1(v)), coef, ss, n))
        Jtw = back(ops.jacobi_fused_bwd(nhw1(w), coef, ss, n))
        lhs, rhs_ = float(np.vdot(Jv, w)), float(np.vdot(v, Jtw))
        print('adjoint identity %s n=%d: %.10e vs %.10e' % (list(ss), n, lhs, rhs_))
        assert abs(lhs - rhs_) <= 1e-5 * max(abs(lhs), abs(rhs_))


def test_fused_3x3_against_the_per_sweep_kernel():
    """(d) The two routes sum in different orders: compared at the oracle's bound.  The default-constructed layer IS the per-sweep path, bit for bit."""
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    ss, od = (3, 3), (2, 2)
    H, W = shapes(ss)[3]
    u, rhs, dx, dout = inputs(H, W)
    ud, rd, dd, dxd = nhw1(u), nhw1(rhs), nhw1(dout), dev(dx)
    ref = references(ss, od, H, W)
    for n in (1, sweep_counts(ss)[2]):
        a, b = ud, dd
        for _ in range(n):
            a = ops.jacobi_sweep(a, rd, dxd)
            b = ops.jacobi_sweep_bwd(b, dxd)
        fused = JacobiIterationLayer(n, fused=True)
        yf = fused.forward(ud, rd, dxd)
        df = fused.backward(dd)
        print('fused vs per-sweep n=%d: fwd %.2e bwd %.2e' % (n, rel(back(yf), back(a)), rel(back(df), back(b))))
        assert rel(back(yf), back(a)) < bound(n, ref[n][2]) and rel(back(df), back(b)) < bound(n, ref[n][3])
        default = JacobiIterationLayer(n)
        assert torch.equal(default.forward(ud, rd, dxd), a) and torch.equal(default.backward(dd), b)


def test_the_harness_rejects_wrong_twins():
    """(e) The same data, bounds and rel() as above must tell these three wrong twins from the kernel, else passing them proves nothing."""
    H, W = 11, 13
    u, rhs, dx, _ = inputs(H, W)
    # the fp64 recurrence with the right rows IS the oracle
    for ss, od in (((3, 7), (2, 2)), ((5, 7), (4, 2))):
        assert rel(recurrence(u, rhs, rows_of(ss, od, dx, np.float64), ss, 2, np.float64), np_ops.jacobi_iterations(u, rhs, dx, 2, ss, od)) < 1e-13
    ss, od = (3, 7), (2, 2)
    ref = references(ss, od, H, W)
    r64 = rows_of(ss, od, dx, np.float64)
    for k in sweep_counts(ss)[:2]:
        got = gpu_fwd(ss, od, H, W, k)
        b = bound(k, ref[k][2])                                    # the very bound test (a) applies to this case
        assert rel(got, recurrence(u, rhs, r64, ss, k, np.float64)) < b
        # H and W taps exchanged: the 7-point line (and its dx) along H, the 3-point line along W
        assert rel(got, np_ops.jacobi_iterations(u, rhs, dx[:, ::-1], k, (7, 3), od)) > b
        # the ring one point too narrow along W
        assert rel(got, recurrence(u, rhs, r64, ss, k, np.float64, ring=(1, 2))) > b
        # 1 / diagonal from the transposed dx
        wrong = r64.copy()
        wrong[:, -1] = rows_of(ss, od, dx[:, ::-1], np.float64)[:, -1]
        assert rel(got, recurrence(u, rhs, wrong, ss, k, np.float64)) > b


@pytest.mark.parametrize('data_format', ['channels_first', 'channels_last'])
def test_keras_layer_on_the_tape(data_format):
    """(f) K.JacobiIterationLayer([5,5],[2,2],n_iterations=3) through autograd.Differentiable == its hand-chained backward, bit for bit, and the
    oracle's values."""
    from poisson_cnn_amd import keras_layers as K
    from poisson_cnn_amd.autograd import Differentiable
    H, W = 21, 18
    u, rhs, dx, dout = inputs(H, W)
    cl = data_format == 'channels_last'
    put = (lambda a: dev(a.transpose(0, 2, 3, 1))) if cl else dev
    g, r, dy, dxd = put(u), put(rhs), put(dout), dev(dx)
    a, b = [K.JacobiIterationLayer([5, 5], [2, 2], n_iterations=3, data_format=data_format) for _ in range(2)]
    ya = a.call([g, r, dxd], training=True)
    da = a.backward(dy)
    mod = Differentiable(b)
    gb = g.clone().requires_grad_(True)
    yb = mod([gb, r, dxd])
    yb.backward(dy)
    assert tuple(ya.shape) == tuple(g.shape) and torch.equal(ya, yb) and torch.equal(gb.grad, da)
    get = (lambda t: t.cpu().numpy().transpose(0, 3, 1, 2)) if cl else (lambda t: t.cpu().numpy())
    ut = torch.tensor(u, requires_grad=True)
    yt = torch_twin.jacobi_iterations(ut, rhs, dx, 3, (5, 5), (2, 2))
    (yt * torch.tensor(dout)).sum().backward()
    r32 = rows_of((5, 5), (2, 2), dx, np.float32)
    e_f = rel(recurrence(u, rhs, r32, (5, 5), 3, np.float32), yt.detach().numpy())
    e_b = rel(recurrence(dout, rhs, r32, (5, 5), 3, np.float32, adjoint=True), ut.grad.numpy())
    assert rel(get(ya.detach()), yt.detach().numpy()) < bound(3, e_f) and rel(get(da), ut.grad.numpy()) < bound(3, e_b)
    # dx as one column means dx == dy
    dx1 = np.concatenate([dx[:, :1]] * 2, 1)
    y1 = K.JacobiIterationLayer(5, 2, n_iterations=2, data_format=data_format).call([g, r, dxd[:, :1]])
    o1 = np_ops.jacobi_iterations(u, rhs, dx1, 2, (5, 5), (2, 2))
    assert rel(get(y1), o1) < bound(2, rel(recurrence(u, rhs, rows_of((5, 5), (2, 2), dx1, np.float32), (5, 5), 2, np.float32), o1))


@pytest.mark.parametrize('ss', [[5, 3], [3, 7]])
@pytest.mark.parametrize('H,W', [(17, 12), (40, 33)])
def test_physics_informed_loss_with_rectangular_stencils(ss, H, W):
    """(g) loss value and dL/dpred against oracle/loss.py, at the tolerances tests/test_gpu_ops.py applies to loss_wrapper (2e-5 relative on the value,
    5e-6 rel-L2 on the gradient)."""
    from poisson_cnn_amd.losses import loss_wrapper
    rng = np.random.default_rng(H + ss[0])
    yt, yp = f32(rng.standard_normal((N, 1, H, W))), f32(rng.standard_normal((N, 1, H, W)))
    rhs = f32(rng.standard_normal((N, 1, H, W)))
    dx = f32(rng.uniform(5e-3, 5e-2, (N, 2)))
    cfg = dict(ndims=2, integral_loss_weight=0.7, integral_loss_config={'n_quadpts': 9}, physics_informed_loss_weight=6e-4,
               physics_informed_loss_config={'stencil_sizes': ss, 'orders': [2, 2], 'normalize': H == 40}, mse_loss_weight=0.2, mae_loss_weight=0.1,
               global_batch_size=6)
    ypt = torch.tensor(yp, requires_grad=True)
    ref = oloss.loss_wrapper(**cfg)(yt, ypt, torch.tensor(rhs), dx)
    ref.backward()
    loss, dpred = loss_wrapper(**cfg)._evaluate(dev(yt), dev(yp), dev(rhs), dev(dx), True)
    ev, eg = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach())), rel(dpred.cpu().numpy(), ypt.grad.numpy())
    print('pi loss %s %dx%d: value %.2e gradient %.2e' % (ss, H, W, ev, eg))
    assert ev < 2e-5 and eg < 5e-6


def test_square_stencil_through_both_loss_entry_points():
    """(g) [5,5]: pcnn_pi_loss_partials / _bwd (one int s) and the _rect entry points give the same bits."""
    from ctypes import c_int
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.losses import loss_wrapper
    H, W = 40, 33
    rng = np.random.default_rng(5)
    yp, rhs = dev(rng.standard_normal((N, 1, H, W))), dev(rng.standard_normal((N, 1, H, W)))
    L = loss_wrapper(ndims=2, integral_loss_weight=0.0, integral_loss_config={'n_quadpts': 9}, physics_informed_loss_weight=1.0,
                     physics_informed_loss_config={'stencil_sizes': [5, 5], 'orders': [2, 2]})
    kern = L._pi_kernels(dev(rng.uniform(5e-3, 5e-2, (N, 2))), H, W)
    coef = dev(rng.uniform(0.5, 1.0, (N,)))
    new = ops.pi_loss_partials(yp, rhs, kern)
    dnew = ops.pi_loss_bwd(yp, rhs, kern, coef, torch.zeros_like(yp))
    old, dold = torch.empty_like(new), torch.zeros_like(yp)
    h = ops.handle()
    h.call('pcnn_pi_loss_partials', c_int(N), c_int(H), c_int(W), c_int(5), ops._p(yp), ops._p(rhs), ops._p(kern), ops._p(old))
    h.call('pcnn_pi_loss_bwd', c_int(N), c_int(H), c_int(W), c_int(5), ops._p(yp), ops._p(rhs), ops._p(kern), ops._p(coef), ops._p(dold))
    assert torch.equal(new, old) and torch.equal(dnew, dold) and float(new.abs().min()) > 0


def test_refusals():
    """(h) Bad arguments: a non-zero status with a pcnn_last_error message, and nothing launched (the output keeps its sentinel)."""
    from ctypes import c_int
    from poisson_cnn_amd import ops
    H, W = 11, 13
    u, r = ops.zeros((N, H, W, 1)), ops.zeros((N, H, W, 1))
    out = torch.full((N, H, W, 1), 7.0, device='cuda')
    coef = torch.ones((N, 32), device='cuda')
    h = ops.handle()

    def fwd(sy, sx, n, Hh=H, Ww=W, uu=u, rr=r, oo=out):
        h.call('pcnn_jacobi_fused_fwd', c_int(N), c_int(Hh), c_int(Ww), c_int(sy), c_int(sx), ops._p(coef), ops._p(uu), ops._p(rr), c_int(n), ops._p(oo))

    def bwd(sy, sx, n, Hh=H, Ww=W, dd=u, oo=out):
        h.call('pcnn_jacobi_fused_bwd', c_int(N), c_int(Hh), c_int(Ww), c_int(sy), c_int(sx), ops._p(coef), ops._p(dd), c_int(n), ops._p(oo))

    bad = [dict(sy=4, sx=3, n=1), dict(sy=3, sx=6, n=1), dict(sy=11, sx=3, n=1), dict(sy=3, sx=1, n=1), dict(sy=3, sx=3, n=0), dict(sy=3, sx=3, n=-2),
           dict(sy=5, sx=3, n=1, Hh=4), dict(sy=3, sx=7, n=1, Ww=6)]
    for kw in bad:
        for fn, name in ((fwd, 'pcnn_jacobi_fused_fwd'), (bwd, 'pcnn_jacobi_fused_bwd')):
            with pytest.raises(RuntimeError, match=name):
                fn(**kw)
    with pytest.raises(RuntimeError, match='alias'):
        fwd(3, 3, 1, oo=u)
    with pytest.raises(RuntimeError, match='alias'):
        fwd(3, 3, 1, oo=r)
    with pytest.raises(RuntimeError, match='alias'):
        bwd(3, 3, 1, oo=u)
    with pytest.raises(RuntimeError, match='null'):
        fwd(3, 3, 1, rr=None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((u == 0).all()) and bool((r == 0).all())
    fwd(3, 3, 1)                                                   # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool((out == 0).all())
