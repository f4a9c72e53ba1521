"""Training-mode BatchNormalization kernels (ops.bn_train_forward / bn_train_backward / channel_affine, csrc/pointwise.hip) called directly, against
the fp64 oracle (np_ops.batchnorm_training; autograd of torch_twin.batchnorm_training), channel by channel, on inputs whose channels sit at
|mean|/std = 0, 3, 30, 100, 300 and on an exactly constant channel.  Inputs, reference, bounds and their derivation: tests/bn_bounds.py;
tests/test_bn_stats_reference.py shows on the CPU that these bounds reject the one-pass sum a, sum a*a statistics."""
import functools

import numpy as np
import pytest
import torch

from tests import bn_bounds as B

pytestmark = pytest.mark.gpu
SENTINEL = 123.0


@functools.lru_cache(maxsize=None)
def _case(name):
    case = B.make_case(name)
    return case, B.reference(case)          # computed once per shape, shared by the forward and backward tests, never modified


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda')


def host(t):
    return t.detach().cpu().numpy()


def _activation(name, case):
    """The activation on the device: contiguous, or a channel window of a wider buffer whose other channels hold NaN."""
    window = B.SHAPES[name][1]
    if window is None:
        return dev(case['a'])
    ld, off = window
    C = case['a'].shape[-1]
    buf = torch.full(case['a'].shape[:3] + (ld,), float('nan'), dtype=torch.float32, device='cuda')
    buf[..., off:off + C] = dev(case['a'])
    return buf[..., off:off + C]


def _forward(name, case, residual=None, out=None):
    from poisson_cnn_amd import ops
    mm, mv = dev(case['moving_mean']), dev(case['moving_var'])
    y, (mean, inv_std, scale) = ops.bn_train_forward(_activation(name, case), dev(case['gamma']), dev(case['beta']), mm, mv, residual=residual, out=out)
    torch.cuda.synchronize()
    return dict(y=host(y), mean=host(mean), inv_std=host(inv_std), scale=host(scale), moving_mean=host(mm), moving_var=host(mv))


def _report(name, case, ref, got, bwd=None):
    """One line per |ratio| of the tensor: the largest relative error of the variance (through inv_std), of y and of dgamma."""
    C = case['a'].shape[-1]
    var_rel = 2 * np.abs(got['inv_std'] - ref['inv_std']) / ref['inv_std'] * (ref['var'] + B.EPS) / np.maximum(ref['var'], 1e-300)
    gx = np.sqrt(((case['gamma'] * ref['xhat']).reshape(-1, C) ** 2).sum(0))
    y_rel = np.sqrt(((got['y'] - ref['y']).reshape(-1, C) ** 2).sum(0)) / np.maximum(gx, 1e-300)
    for r in sorted(set(np.abs(case['ratio'][~case['const']]))):
        sel = (np.abs(case['ratio']) == r) & ~case['const']
        line = 'BNERR %-16s ratio %5g  var %.2e  y %.2e' % (name, r, var_rel[sel].max(), y_rel[sel].max())
        if bwd is not None:
            line += '  dgamma %.2e' % (np.abs(bwd['dgamma'] - ref['dgamma'])[sel] / np.abs(ref['dgamma'][sel])).max()
        print(line)


@pytest.mark.parametrize('name', sorted(B.SHAPES))
def test_forward_statistics_and_output(name):
    case, ref = _case(name)
    C = case['a'].shape[-1]
    got = _forward(name, case)
    _report(name, case, ref, got)
    checks = B.forward_checks(case, ref, got)
    print('worst err/bound', B.worst(checks))
    assert B.violations(checks) == []
    if case['const'].any():        # variance exactly 0, never negative: inv_std = 1/sqrt(eps), the moving variance only decays
        c = case['const']
        assert np.all(np.abs(got['inv_std'][c] * np.sqrt(B.EPS) - 1) <= 4 * B.U)
        assert np.all(got['moving_var'][c] <= np.float32(case['moving_var'][c]) * np.float32(B.MOMENTUM))
    assert np.isfinite(got['y']).all()
    # + residual; out= given (a channel window of a wider buffer, whose other channels must stay as they were); out= the residual itself (layers.py)
    res = dev(case['residual'])
    wide = torch.full(case['a'].shape[:3] + (C + 5,), SENTINEL, dtype=torch.float32, device='cuda')
    alias = res.clone()
    variants = {'residual': _forward(name, case, residual=res), 'out': _forward(name, case, out=wide[..., 2:2 + C]),
                'out+residual': _forward(name, case, residual=res, out=wide[..., 2:2 + C]), 'out=residual': _forward(name, case, residual=alias, out=alias)}
    assert torch.equal(res, dev(case['residual'])) and bool((wide[..., :2] == SENTINEL).all()) and bool((wide[..., 2 + C:] == SENTINEL).all())
    for what, g in variants.items():
        checks = B.forward_checks(case, ref, g, residual=None if what == 'out' else case['residual'])
        assert B.violations(checks) == [], what
        for k in ('mean', 'inv_std', 'scale', 'moving_mean', 'moving_var'):      # the reductions are deterministic
            assert np.array_equal(g[k], got[k]), (what, k)
    assert np.array_equal(variants['out=residual']['y'], variants['residual']['y']) and np.array_equal(host(alias), variants['residual']['y'])


@pytest.mark.parametrize('name', sorted(B.SHAPES))
def test_backward(name):
    from poisson_cnn_amd import ops
    case, ref = _case(name)
    C = case['a'].shape[-1]
    a = _activation(name, case)
    _, stats = ops.bn_train_forward(a, dev(case['gamma']), dev(case['beta']), dev(case['moving_mean']), dev(case['moving_var']))
    dgamma, dbeta = torch.full((C,), SENTINEL, device='cuda'), torch.full((C,), SENTINEL, device='cuda')
    da = ops.bn_train_backward(dev(case['dy']), a, stats, dgamma, dbeta)
    torch.cuda.synchronize()
    got = dict(da=host(da), dgamma=host(dgamma), dbeta=host(dbeta))
    _report(name, case, ref, dict(y=ref['y'], inv_std=host(stats[1])), got)      # (the y column of these lines is 0: no y here)
    checks = B.backward_checks(case, ref, got)
    print('worst err/bound', B.worst(checks))
    assert B.violations(checks) == []
    assert np.isfinite(got['da']).all()


def test_more_than_256_channels_is_refused_before_any_launch():
    from poisson_cnn_amd import ops
    C = 257
    a = torch.ones((1, 2, 2, C), device='cuda')
    mm, mv, out = (torch.full(s, SENTINEL, device='cuda') for s in ((C,), (C,), (1, 2, 2, C)))
    with pytest.raises(RuntimeError, match='C=257 unsupported'):
        ops.bn_train_forward(a, torch.ones(C, device='cuda'), torch.ones(C, device='cuda'), mm, mv, out=out)
    stats = tuple(torch.ones(C, device='cuda') for _ in range(3))
    dg, db = torch.full((C,), SENTINEL, device='cuda'), torch.full((C,), SENTINEL, device='cuda')
    with pytest.raises(RuntimeError, match='C=257 unsupported'):
        ops.bn_train_backward(a, a, stats, dg, db)
    torch.cuda.synchronize()
    for t in (mm, mv, out, dg, db):
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize('with_residual', [False, True])
@pytest.mark.parametrize('C', [1, 6, 8])
def test_channel_affine(C, with_residual):
    """y = x*scale + shift (+ residual) into a channel window of a wider buffer; the channels around the window stay untouched."""
    from poisson_cnn_amd import ops
    rng = np.random.default_rng(C)
    shape = (2, 5, 7, C)
    x, res = B.f32(rng.standard_normal(shape)), B.f32(rng.standard_normal(shape))
    scale, shift = B.f32(rng.uniform(0.5, 2.0, C) * np.where(np.arange(C) % 2, -1, 1)), B.f32(rng.standard_normal(C))
    wide = torch.full(shape[:3] + (C + 5,), SENTINEL, dtype=torch.float32, device='cuda')
    y = ops.channel_affine(dev(x), dev(scale), dev(shift), residual=dev(res) if with_residual else None, out=wide[..., 3:3 + C])
    torch.cuda.synchronize()
    ref = x * scale + shift + (res if with_residual else 0.0)
    # three fp32 roundings per element, each at most u times the larger of the partial results
    assert y.data_ptr() == wide[..., 3:3 + C].data_ptr()
    assert np.all(np.abs(host(y) - ref) <= 3 * B.U * (np.abs(x * scale) + np.abs(shift) + np.abs(res) * with_residual))
    assert bool((wide[..., :3] == SENTINEL).all()) and bool((wide[..., 3 + C:] == SENTINEL).all())
    fresh = ops.channel_affine(dev(x), dev(scale), dev(shift), residual=dev(res) if with_residual else None)
    assert fresh.is_contiguous() and torch.equal(fresh, y)
