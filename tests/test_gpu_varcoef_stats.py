"""pcnn_varcoef_error_stats (csrc/error_stats.hip, ops.varcoef_error_stats) against tests/error_stats_twin.py on the same fp32 inputs."""
from ctypes import c_int

import numpy as np
import pytest
import torch

from tests import error_stats_twin as TW

pytestmark = pytest.mark.gpu

N = 3
# 3 x 3: one interior point; 5 x 67: the lanes' column stride (64) is taken twice; 70 x 5: more rows than the 64 bands, so a band holds two rows;
# 130 x 33: three rows per band - band edges inside the image, the neighbour rows of a band's first and last row belong to other workgroups.
SHAPES = [(3, 3), (5, 67), (70, 5), (130, 33)]
EPS = 2.0 ** -23
# The sums, against the twin that forms every term (e, t, r, f) in float32 in the kernel's own operation order and adds in float64.  All terms of a
# sum are non-negative, so its relative error is at most (longest addition chain + roundings that form one term from those float32 values) * eps.
# The kernel's decomposition (64 bands of rows per sample, 16 waves per band, one row per wave at a time, lanes stride the columns by 64):
#   per lane ceil(ceil(H / 64) / 16) * ceil(W / 64) additions - 2 at 5 x 67, the most here -, 6 butterfly steps over the wave's lanes, 15 additions
#   over the band's waves, 6 butterfly steps over the bands: 29 additions; the term itself is one more rounding (e * e, t * t, r * r, f * f; |e| none).
SUM_TOL = 30 * EPS
# max|r| against the float64 twin, a bound on the rounding of one point.  With u = EPS / 2 the unit roundoff, to first order:
#   b_k = 2 / (rc + r_k): 2 roundings, d_k = u_k - uc: 1, b_k d_k: 1 -> each product is off by 4u of itself, and |b_k d_k| <= (1 / min rho) 2 max|p|;
#   three additions: 3u of the sum of the four |products|;  1 / (dx dx): 2 roundings, the multiplication by it: 1  -> 10u of 8 max|p| / (min rho dx^2);
#   the subtraction of f: u (8 max|p| / (min rho dx^2) + max|f|).
# Taken with EPS = 2u in place of u, which covers the second-order terms:  11 EPS 8 max|p| / (min rho dx^2) + EPS max|f|.
SUMS, MAXES = (0, 1, 3, 5, 7), (2, 4)


def _inputs(H, W, seed=0):
    rng = np.random.default_rng(1000 * H + W + seed)
    pred = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    target = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    rho = rng.uniform(1.0, 10.0, (N, H, W)).astype(np.float32)
    rhs = (rng.standard_normal((N, H, W)) * 50).astype(np.float32)           # independent of pred: the residual does not cancel
    dx = rng.uniform(5e-3, 5e-2, (N,)).astype(np.float32)                   # one spacing per sample, all different
    return pred, target, rho, rhs, dx


_CACHE = {}


def _call(ops, pred, target, rho, rhs, dx):
    return ops.varcoef_error_stats(pred, rho, target, rhs, dx)


def _case(H, W):
    """(inputs, device tensors, the kernel's (N, 8) rows, the float32-term twin's, the float64 twin's) - computed once per shape and shared"""
    if (H, W) not in _CACHE:
        from poisson_cnn_amd import ops
        arrs = _inputs(H, W)
        dev = [torch.from_numpy(a).cuda() for a in arrs]
        got = _call(ops, *dev).cpu().numpy()
        pred, target, rho, rhs, dx = arrs
        _CACHE[(H, W)] = (arrs, dev, got, TW.error_stats(pred, target, rhs, dx, rho, float32_terms=True), TW.error_stats(pred, target, rhs, dx, rho))
    return _CACHE[(H, W)]


bits = lambda a: a.view(np.uint32)


@pytest.mark.parametrize('H,W', SHAPES)
def test_matches_the_twins(H, W):
    (pred, target, rho, rhs, dx), _, got, ref32, ref64 = _case(H, W)
    assert got.shape == (N, 8) and got.dtype == np.float32
    # maxima of e and t: the bits of a float32 numpy evaluation
    assert np.array_equal(got[:, 2], np.abs(pred - target).reshape(N, -1).max(1)) and np.array_equal(got[:, 4], np.abs(target).reshape(N, -1).max(1))
    flat = lambda a: a.reshape(N, -1).astype(np.float64)
    scale = 8 * np.abs(flat(pred)).max(1) / (flat(rho).min(1) * dx.astype(np.float64) ** 2)
    bound = 11 * EPS * scale + EPS * np.abs(flat(rhs)).max(1)
    err_r = np.abs(got[:, 6] - ref64[:, 6])
    rel = np.abs(got[:, SUMS] - ref32[:, SUMS]) / ref32[:, SUMS]
    print('%dx%d: max|r| error / bound %.3g, sums rel. error / tolerance %.3g' % (H, W, (err_r / bound).max(), rel.max() / SUM_TOL))
    assert np.all(err_r <= bound)
    assert np.all(ref32[:, SUMS] > 0) and np.all(rel <= SUM_TOL)


@pytest.mark.parametrize('H,W', SHAPES)
def test_samples_do_not_see_their_neighbours(H, W):
    """Sample 1 filled with 1e30 in all four fields: a neighbour taken from the next sample would show in samples 0 and 2."""
    from poisson_cnn_amd import ops
    _, dev, got, _, _ = _case(H, W)
    big = [t.clone() for t in dev[:4]]
    for t in big:
        t[1] = 1e30
    out = _call(ops, *big, dev[4]).cpu().numpy()
    assert np.array_equal(bits(out[[0, 2]]), bits(got[[0, 2]]))


@pytest.mark.parametrize('H,W', [(5, 67), (130, 33)])
def test_null_fields_layouts_and_determinism(H, W):
    from poisson_cnn_amd import ops
    _, (pred, target, rho, rhs, dx), got, _, _ = _case(H, W)
    assert np.array_equal(bits(_call(ops, pred, target, rho, rhs, dx).cpu().numpy()), bits(got))          # two calls: equal bits
    no_t = ops.varcoef_error_stats(pred, rho, None, rhs, dx).cpu().numpy()
    assert np.all(no_t[:, :5] == 0.0) and np.array_equal(bits(no_t[:, 5:]), bits(got[:, 5:]))
    for r in (rho, None):                                                                                   # without rhs, rho is not read
        no_f = ops.varcoef_error_stats(pred, r, target).cpu().numpy()
        assert np.all(no_f[:, 5:] == 0.0) and np.array_equal(bits(no_f[:, :5]), bits(got[:, :5]))
    assert np.all(ops.varcoef_error_stats(pred, None).cpu().numpy() == 0.0)
    # the (N,1,H,W) and (N,H,W,1) layouts of the models are the same memory
    v1, v3 = (lambda t: t.view(N, 1, H, W)), (lambda t: t.view(N, H, W, 1))
    assert np.array_equal(bits(_call(ops, v1(pred), v1(target), v1(rho), v1(rhs), dx.view(N, 1)).cpu().numpy()), bits(got))
    assert np.array_equal(bits(_call(ops, v3(pred), v3(target), v3(rho), v3(rhs), dx).cpu().numpy()), bits(got))
    assert np.array_equal(bits(_call(ops, v3(pred), target, v1(rho), rhs, dx).cpu().numpy()), bits(got))


def test_argument_errors_leave_the_handle_usable():
    from poisson_cnn_amd import ops
    _, (pred, target, rho, rhs, dx), got, _, _ = _case(5, 67)
    with pytest.raises(ValueError, match='rhs needs rho'):
        ops.varcoef_error_stats(pred, None, target, rhs, dx)
    with pytest.raises(ValueError, match='rhs needs dx'):
        ops.varcoef_error_stats(pred, rho, target, rhs)
    two = [t[:, :2, :5].contiguous() for t in (pred, target, rho, rhs)]
    with pytest.raises(RuntimeError, match='H, W >= 3'):                                    # a 2 x 5 grid has no interior
        _call(ops, *two, dx)
    with pytest.raises(ValueError):
        ops.varcoef_error_stats(pred, rho, target[:, :4].contiguous())
    with pytest.raises(ValueError, match='one spacing per sample'):
        ops.varcoef_error_stats(pred, rho, target, rhs, torch.cat([dx, dx]).view(N, 2))
    # the library itself refuses what the Python layer caught above - an argument error, nothing is launched
    out = ops.empty((N, 8), pred.device)
    dims = (c_int(N), c_int(5), c_int(67))
    for r, d, msg in ((None, dx, 'rhs needs rho'), (rho, None, 'rhs needs dx')):
        with pytest.raises(RuntimeError, match=msg):
            ops.handle().call('pcnn_varcoef_error_stats', *dims, ops._p(pred), ops._p(target), ops._p(r), ops._p(rhs), ops._p(d), ops._p(out))
    ok = ops.varcoef_error_stats(two[0], None, two[1]).cpu().numpy()                        # H = 2 without rhs is fine
    assert np.allclose(ok, TW.error_stats(two[0].cpu().numpy(), two[1].cpu().numpy()), rtol=1e-6)
    assert np.array_equal(bits(_call(ops, pred, target, rho, rhs, dx).cpu().numpy()), bits(got))
