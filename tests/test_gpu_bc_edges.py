"""The per-edge ring (pcnn_bc_ring_edges_fwd/bwd) and the boundary-aware fused smoother (pcnn_jacobi_fused_bc_fwd/bwd) against the twins of
tests/bc_edges_twin.py, which tests/test_bc_edges_reference.py pins to the oracle.

Bounds: the ring is a copy - exact forward, 2e-6 rel-L2 backward (the ring's bound in tests/test_gpu_ops.py).  The smoother follows the rule of
tests/test_gpu_jacobi_stencil.py: 2e-6 for one sweep; beyond, max(2e-6, 4 x the float32-CPU recurrence's own rel-L2 against the fp64 twin, for that very
case).  Every figure is printed before it is asserted.

The smoother entry points are called through the handle for every mask, 0 included (ops.jacobi_fused sends mask 0 to the frozen-band entry point, and so
do the new entry points themselves: DESIGN.md section 11.1).

R_m leaves a band point on a Dirichlet edge frozen where E_m sets it to zero, so "n sweeps == n x (sweep, then ring)" holds for a guess that already
satisfies its Dirichlet condition - the model's does, it comes out of the ring - and is tested on E_m of the random guess."""
import functools
from ctypes import c_int

import numpy as np
import pytest
import torch

from tests import bc_edges_twin as T

pytestmark = pytest.mark.gpu
TOL = 2e-6
N = 2
MASKS = [0, 15, 1, 2, 4, 8, 0b0110]
RING_SHAPES = [(3, 3), (4, 7), (65, 70)]
STENCILS = [((3, 3), (2, 2)), ((5, 7), (4, 2)), ((9, 3), (2, 2))]
SHAPES = [(12, 12), (64, 64), (65, 70), (130, 67)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda')


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def nhw1(a):
    return dev(np.asarray(a)[:, 0, :, :, None])


def back(t):
    return t.detach().cpu().numpy()[:, None, :, :, 0].astype(np.float64)


def sweep_counts(ss):
    from poisson_cnn_amd import ops
    k = ops.jacobi_k_max(*ss)
    return [1, k, k + 1]


@functools.lru_cache(maxsize=None)
def inputs(H, W):
    rng = np.random.default_rng(77 * H + W)
    u = f32(rng.standard_normal((N, 1, H, W)))
    rhs = f32(rng.standard_normal((N, 1, H, W)))
    dx = f32(rng.uniform(5e-3, 5e-2, (N, 2)))                      # a distinct anisotropic row per sample
    dout = f32(rng.standard_normal((N, 1, H, W)))
    return u, rhs, dx, dout                                         # shared: read, never written


def rows32(ss, od, dx):
    from poisson_cnn_amd.layers import JacobiIterationLayer
    return JacobiIterationLayer(1, ss, od).coefficient_rows(torch.from_numpy(dx.astype(np.float32))).numpy()


@functools.lru_cache(maxsize=None)
def references(ss, od, H, W, mask):
    """Per sweep count: the fp64 twin forward and adjoint, and the float32-CPU recurrence's error against each."""
    u, rhs, dx, dout = inputs(H, W)
    r32 = rows32(ss, od, dx)
    out, x, done = {}, u, 0
    for n in sweep_counts(ss):
        x = T.sweeps(x, rhs, dx, n - done, mask, ss, od)
        done = n
        adj = T.adjoint(u, rhs, dx, dout, n, mask, ss, od)
        e_f = rel(T.recurrence(u, rhs, r32, ss, n, mask, np.float32), x)
        e_b = rel(T.recurrence(dout, rhs, r32, ss, n, mask, np.float32, adjoint=True), adj)
        out[n] = (x, adj, e_f, e_b)
    return out


def bound(n, e_cpu32):
    return TOL if n == 1 else max(TOL, 4.0 * e_cpu32)


def coef_of(ss, od, dx):
    from poisson_cnn_amd.layers import JacobiIterationLayer
    return JacobiIterationLayer(1, ss, od).coefficient_rows(dev(dx))


def bc_fwd(u, rhs, coef, ss, n, mask, out=None):
    from poisson_cnn_amd import ops
    Nn, H, W = u.shape[0], u.shape[1], u.shape[2]
    out = torch.empty_like(u) if out is None else out
    ops.handle().call('pcnn_jacobi_fused_bc_fwd', c_int(Nn), c_int(H), c_int(W), c_int(ss[0]), c_int(ss[1]), ops._p(coef), ops._p(u), ops._p(rhs), c_int(n),
                      c_int(mask), ops._p(out))
    return out


def bc_bwd(d, coef, ss, n, mask, out=None):
    from poisson_cnn_amd import ops
    Nn, H, W = d.shape[0], d.shape[1], d.shape[2]
    out = torch.empty_like(d) if out is None else out
    ops.handle().call('pcnn_jacobi_fused_bc_bwd', c_int(Nn), c_int(H), c_int(W), c_int(ss[0]), c_int(ss[1]), ops._p(coef), ops._p(d), c_int(n), c_int(mask),
                      ops._p(out))
    return out


# ------------------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize('H,W', RING_SHAPES)
def test_ring_forward_and_backward(H, W):
    from poisson_cnn_amd import ops
    u, w, _, _ = inputs(H, W)
    for mask in MASKS:
        assert np.array_equal(back(ops.bc_ring_edges_fwd(nhw1(u), mask)), T.ring(u, mask)), mask
        e = rel(back(ops.bc_ring_edges_bwd(nhw1(w), mask)), T.ring_adjoint(w, mask))
        print('ring bwd %dx%d mask %d: %.2e' % (H, W, mask, e))
        assert e < TOL, mask


@pytest.mark.parametrize('H,W', RING_SHAPES)
def test_ring_masks_0_and_15_are_the_old_entry_points(H, W):
    from poisson_cnn_amd import ops
    u, w, _, _ = inputs(H, W)
    ud, wd = nhw1(u), nhw1(w)
    for mask, neumann in ((0, False), (15, True)):
        assert torch.equal(ops.bc_ring_edges_fwd(ud, mask), ops.bc_ring_fwd(ud, neumann))
        assert torch.equal(ops.bc_ring_edges_bwd(wd, mask), ops.bc_ring_bwd(wd, neumann))


# --------------------------------------------------------------------------------------------------------------------- the smoother
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('ss,od', STENCILS)
def test_smoother_against_the_twin(ss, od, mask):
    fails = []
    for (H, W) in SHAPES:
        u, rhs, dx, dout = inputs(H, W)
        ref = references(ss, od, H, W, mask)
        coef = coef_of(ss, od, dx)
        ud, rd, dd = nhw1(u), nhw1(rhs), nhw1(dout)
        for n in sweep_counts(ss):
            xf, xb, e_f, e_b = ref[n]
            g_f, g_b = rel(back(bc_fwd(ud, rd, coef, ss, n, mask)), xf), rel(back(bc_bwd(dd, coef, ss, n, mask)), xb)
            print('bc jacobi %s/%s mask %d %dx%d n=%d: fwd gpu %.2e cpu32 %.2e bound %.2e | bwd gpu %.2e cpu32 %.2e bound %.2e'
                  % (list(ss), list(od), mask, H, W, n, g_f, e_f, bound(n, e_f), g_b, e_b, bound(n, e_b)))
            if not g_f < bound(n, e_f):
                fails.append(('fwd', H, W, n, g_f, bound(n, e_f)))
            if not g_b < bound(n, e_b):
                fails.append(('bwd', H, W, n, g_b, bound(n, e_b)))
    assert not fails, fails


@pytest.mark.parametrize('ss,od', STENCILS)
def test_fusing_is_exact_and_mask_0_is_the_frozen_kernel(ss, od):
    """n sweeps in as few launches as possible == n launches of one sweep, bit for bit, forward and adjoint, for every mask and shape; and mask 0 through
    the new entry points == ops.jacobi_fused / jacobi_fused_bwd."""
    from poisson_cnn_amd import ops
    for (H, W) in SHAPES:
        u, rhs, dx, dout = inputs(H, W)
        coef = coef_of(ss, od, dx)
        ud, rd, dd = nhw1(u), nhw1(rhs), nhw1(dout)
        for n in sweep_counts(ss):
            for mask in MASKS:
                a, b = ud, dd
                for _ in range(n):
                    a = bc_fwd(a, rd, coef, ss, 1, mask)
                    b = bc_bwd(b, coef, ss, 1, mask)
                assert torch.equal(bc_fwd(ud, rd, coef, ss, n, mask), a), (H, W, n, mask)
                assert torch.equal(bc_bwd(dd, coef, ss, n, mask), b), (H, W, n, mask)
            assert torch.equal(bc_fwd(ud, rd, coef, ss, n, 0), ops.jacobi_fused(ud, rd, coef, ss, n)), (H, W, n)
            assert torch.equal(bc_bwd(dd, coef, ss, n, 0), ops.jacobi_fused_bwd(dd, coef, ss, n)), (H, W, n)


def test_3x3_sweeps_are_sweep_then_ring():
    from poisson_cnn_amd import ops
    ss, od = (3, 3), (2, 2)
    for (H, W) in SHAPES:
        u, rhs, dx, _ = inputs(H, W)
        coef = coef_of(ss, od, dx)
        rd = nhw1(rhs)
        for mask in MASKS:
            u0 = ops.bc_ring_edges_fwd(nhw1(u), mask)               # a guess that satisfies its Dirichlet condition (module docstring)
            for n in sweep_counts(ss):
                a = u0
                for _ in range(n):
                    a = ops.bc_ring_edges_fwd(ops.jacobi_fused(a, rd, coef, ss, 1), mask)
                assert torch.equal(bc_fwd(u0, rd, coef, ss, n, mask), a), (H, W, n, mask)
                assert torch.equal(ops.jacobi_fused(u0, rd, coef, ss, n, neumann_mask=mask), a), (H, W, n, mask)


@pytest.mark.parametrize('ss,od', STENCILS)
def test_adjoint_identity(ss, od):
    """<(R J)^n v, w> == <v, adjoint w> with the forward at rhs = 0; fp32 device results, the inner products in fp64 on the host, 1e-5 relative."""
    H, W = SHAPES[3]
    v, _, dx, w = inputs(H, W)
    coef = coef_of(ss, od, dx)
    vd, wd = nhw1(v), nhw1(w)
    for mask in MASKS:
        for n in (1, sweep_counts(ss)[2]):
            Jv = back(bc_fwd(vd, torch.zeros_like(vd), coef, ss, n, mask))
            Jtw = back(bc_bwd(wd, coef, ss, n, mask))
            lhs, rhs_ = float(np.vdot(Jv, w)), float(np.vdot(v, Jtw))
            print('bc adjoint identity %s mask %d n=%d: %.10e vs %.10e' % (list(ss), mask, n, lhs, rhs_))
            assert abs(lhs - rhs_) <= 1e-5 * max(abs(lhs), abs(rhs_))


def test_refusals():
    """A non-zero status with a pcnn_last_error message, and nothing launched (the output keeps its sentinel)."""
    from poisson_cnn_amd import ops
    H, W = 11, 13
    u, r = ops.zeros((N, H, W, 1)), ops.zeros((N, H, W, 1))
    out = torch.full((N, H, W, 1), 7.0, device='cuda')
    coef = torch.ones((N, 32), device='cuda')
    for fn, name in ((lambda **kw: bc_fwd(kw.get('u', u), kw.get('r', r), coef, kw['ss'], 1, kw['mask'], out=kw.get('out', out)), 'pcnn_jacobi_fused_bc_fwd'),
                     (lambda **kw: bc_bwd(kw.get('u', u), coef, kw['ss'], 1, kw['mask'], out=kw.get('out', out)), 'pcnn_jacobi_fused_bc_bwd')):
        for ss, mask in (((9, 3), 1), ((9, 3), 2), ((9, 3), 0b0110), ((3, 3), 16), ((3, 3), -1)):       # H = 11 < 3 * 4 with a y edge set; a mask outside 0..15
            with pytest.raises(RuntimeError, match=name):
                fn(ss=ss, mask=mask)
        with pytest.raises(RuntimeError, match='alias'):
            fn(ss=(3, 3), mask=1, out=u)
    dims = (c_int(N), c_int(H), c_int(W), c_int(3), c_int(3))
    with pytest.raises(RuntimeError, match='null'):
        ops.handle().call('pcnn_jacobi_fused_bc_fwd', *dims, ops._p(coef), ops._p(u), ops._p(None), c_int(1), c_int(1), ops._p(out))
    with pytest.raises(RuntimeError, match='null'):
        ops.handle().call('pcnn_jacobi_fused_bc_bwd', *dims, ops._p(coef), ops._p(None), c_int(1), c_int(1), ops._p(out))
    w_small = ops.zeros((N, H, 11, 1))
    with pytest.raises(RuntimeError, match='pcnn_jacobi_fused_bc_fwd'):                                      # W = 11 < 3 * 4 with an x edge set
        bc_fwd(w_small, w_small, coef, (3, 9), 1, 8, out=torch.empty_like(w_small))
    for name in ('pcnn_bc_ring_edges_fwd', 'pcnn_bc_ring_edges_bwd'):
        with pytest.raises(RuntimeError, match=name):
            ops.handle().call(name, c_int(N), c_int(H), c_int(W), c_int(16), ops._p(u), ops._p(out))
        with pytest.raises(RuntimeError, match='null'):
            ops.handle().call(name, c_int(N), c_int(H), c_int(W), c_int(1), ops._p(u), ops._p(None))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((u == 0).all()) and bool((r == 0).all())
    bc_fwd(u, r, coef, (3, 9), 1, 12, out=out)                       # and a legal call runs
    torch.cuda.synchronize()
    assert bool((out == 0).all())
