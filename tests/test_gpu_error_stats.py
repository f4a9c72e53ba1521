"""pcnn_error_stats (csrc/error_stats.hip, ops.error_stats) against its fp64 twin on the same fp32 inputs."""
import numpy as np
import pytest
import torch

from tests import error_stats_twin as TW

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [(3, 3), (3, 40), (40, 3), (5, 7), (33, 65), (130, 257), (384, 384)]
EPS = 2.0 ** -23
# The sums: every term is non-negative, so the relative error is bounded by (longest addition chain + roundings that form one term) * eps.
# The kernel's decomposition (64 bands of rows per sample, 16 waves per band, one row per wave at a time, lanes stride the columns by 64):
#   per lane ceil(ceil(H / 64) / 16) * ceil(W / 64) additions - 6 at 384 x 384, the largest here -, 6 butterfly steps over the wave's lanes,
#   15 additions over the band's waves, 6 butterfly steps over the bands: 33 additions; forming a term (e, e^2; the five-point residual, r^2) is
#   at most 7 more roundings of that size.  40 eps = 4.8e-6 (the issue's figure for a chain of unknown length was 1e-5).
SUM_TOL = 40 * EPS
SUMS, MAXES = (0, 1, 3, 5, 7), (2, 4)


def _inputs(H, W, seed=0):
    rng = np.random.default_rng(1000 * H + W + seed)
    pred = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    target = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    rhs = (rng.standard_normal((N, H, W)) * 50).astype(np.float32)           # independent of pred: the residual does not cancel
    dx = rng.uniform(5e-3, 5e-2, (N, 2)).astype(np.float32)
    dx[:, 1] = np.where(np.abs(dx[:, 1] - dx[:, 0]) < 1e-3, dx[:, 0] * 1.5, dx[:, 1])
    return pred, target, rhs, dx


_CACHE = {}


def _case(H, W):
    """(inputs, device tensors, the kernel's (N, 8) rows, the twin's) - computed once per shape and shared by the tests below"""
    if (H, W) not in _CACHE:
        from poisson_cnn_amd import ops
        arrs = _inputs(H, W)
        dev = [torch.from_numpy(a).cuda() for a in arrs]
        got = ops.error_stats(*dev).cpu().numpy()
        _CACHE[(H, W)] = (arrs, dev, got, TW.error_stats(*arrs))
    return _CACHE[(H, W)]


@pytest.mark.parametrize('H,W', SHAPES)
def test_matches_the_fp64_twin(H, W):
    (pred, target, rhs, dx), _, got, ref = _case(H, W)
    assert got.shape == (N, 8) and got.dtype == np.float32
    # maxima of e and t: the bits of a float32 numpy evaluation
    e32 = pred - target
    assert np.array_equal(got[:, 2], np.abs(e32).reshape(N, -1).max(1)) and np.array_equal(got[:, 4], np.abs(target).reshape(N, -1).max(1))
    # max|r|: the derived per-point bound
    s = (1.0 / dx.astype(np.float64) ** 2).sum(1)
    bound = 8 * EPS * 4 * np.abs(pred).reshape(N, -1).max(1) * s + EPS * np.abs(rhs).reshape(N, -1).max(1)
    err_r = np.abs(got[:, 6] - ref[:, 6])
    rel = np.abs(got[:, SUMS] - ref[:, SUMS]) / ref[:, SUMS]
    print('%dx%d: max|r| error / bound %.3g, sums rel. error / tolerance %.3g' % (H, W, (err_r / bound).max(), rel.max() / SUM_TOL))
    assert np.all(err_r <= bound)
    assert np.all(ref[:, SUMS] > 0) and np.all(rel <= SUM_TOL)


@pytest.mark.parametrize('H,W', SHAPES)
def test_samples_do_not_see_their_neighbours(H, W):
    """Sample 1 filled with 1e30 in all three fields: a halo row taken from the neighbouring sample would show in samples 0 and 2."""
    from poisson_cnn_amd import ops
    _, dev, got, _ = _case(H, W)
    big = [t.clone() for t in dev[:3]]
    for t in big:
        t[1] = 1e30
    out = ops.error_stats(big[0], big[1], big[2], dev[3]).cpu().numpy()
    assert np.array_equal(out[[0, 2]].view(np.uint32), got[[0, 2]].view(np.uint32))


@pytest.mark.parametrize('H,W', [(5, 7), (130, 257)])
def test_null_fields_and_determinism(H, W):
    from poisson_cnn_amd import ops
    _, (pred, target, rhs, dx), got, _ = _case(H, W)
    bits = lambda a: a.view(np.uint32)
    assert np.array_equal(bits(ops.error_stats(pred, target, rhs, dx).cpu().numpy()), bits(got))          # two calls: equal bits
    no_t = ops.error_stats(pred, None, rhs, dx).cpu().numpy()
    assert np.all(no_t[:, :5] == 0.0) and np.array_equal(bits(no_t[:, 5:]), bits(got[:, 5:]))
    no_f = ops.error_stats(pred, target).cpu().numpy()
    assert np.all(no_f[:, 5:] == 0.0) and np.array_equal(bits(no_f[:, :5]), bits(got[:, :5]))
    only = ops.error_stats(pred).cpu().numpy()
    assert np.all(only == 0.0)
    # the (N,1,H,W) and (N,H,W,1) layouts of the models are the same memory
    assert np.array_equal(bits(ops.error_stats(pred.view(N, 1, H, W), target.view(N, 1, H, W), rhs.view(N, 1, H, W), dx).cpu().numpy()), bits(got))
    assert np.array_equal(bits(ops.error_stats(pred.view(N, H, W, 1), target, rhs, dx).cpu().numpy()), bits(got))


def test_argument_errors_leave_the_handle_usable():
    from poisson_cnn_amd import ops
    _, (pred, target, rhs, dx), got, _ = _case(5, 7)
    with pytest.raises(RuntimeError, match='H, W >= 3'):
        ops.error_stats(pred[:, :2].contiguous(), target[:, :2].contiguous(), rhs[:, :2].contiguous(), dx)
    with pytest.raises(ValueError):
        ops.error_stats(pred, target, rhs)                                   # rhs without dx
    with pytest.raises(ValueError):
        ops.error_stats(pred, target[:, :4].contiguous())
    ok = ops.error_stats(pred[:, :2].contiguous(), target[:, :2].contiguous()).cpu().numpy()      # H = 2 without rhs is fine
    assert np.allclose(ok, TW.error_stats(pred[:, :2].cpu().numpy(), target[:, :2].cpu().numpy()), rtol=1e-6)
    assert np.array_equal(ops.error_stats(pred, target, rhs, dx).cpu().numpy(), got)
