"""clipnorm / global_clipnorm / clipvalue / decay of train.Adam and train.SGD on the GPU (csrc/grad_clip.hip) against the fp64 twin and its
derived bounds (tests/grad_clip_twin.py).  One synthetic bucket of 7952 floats: variable sizes 1 ... 4099, so offsets are no multiples of 4 and
one variable spans two items; it sits 3 floats into a guarded buffer, so its base is not 16-byte aligned either.

The optimizer step is outside graphs.GraphedTrainStep's capture (graphs.py: it stays eager), so there is no capture case here."""
import types

import numpy as np
import pytest
import torch

from tests import grad_clip_twin as T

pytestmark = pytest.mark.gpu
C = 1.0
GUARD = 3
GUARD_VALUE = 12345.678
N = sum(T.SIZES)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def guarded(gvars):
    """(buffer, bucket view) - GUARD floats of GUARD_VALUE on both sides of the bucket."""
    buf = torch.full((N + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device='cuda')
    buf[GUARD:GUARD + N] = torch.from_numpy(np.concatenate(gvars))
    return buf, buf[GUARD:GUARD + N]


def guards_intact(buf):
    return bool((buf[:GUARD] == np.float32(GUARD_VALUE)).all() and (buf[-GUARD:] == np.float32(GUARD_VALUE)).all())


def per_element(per_var):
    return torch.repeat_interleave(per_var[:len(T.SIZES)], torch.tensor(T.SIZES, device=per_var.device))


def f32t(x):
    return torch.tensor(x, dtype=torch.float32, device='cuda')


@pytest.fixture(scope='module')
def bucket():
    return T.make_bucket(C)


@pytest.fixture(scope='module')
def plan():
    from poisson_cnn_amd import ops
    return ops.grad_clip_plan(T.SIZES)


def make_store(gvars, seed=100):
    """What train._Optimizer.bind needs of a layers.ParamStore: flat_w, flat_g and the spec list."""
    n = sum(len(v) for v in gvars)
    w = torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32)).cuda()
    g = torch.from_numpy(np.concatenate(gvars).astype(np.float32)).cuda()
    return types.SimpleNamespace(flat_w=w, flat_g=g, specs=[('v%d' % i, (len(v),), 'zeros', 'w') for i, v in enumerate(gvars)])


# ---------------------------------------------------------------------------------------------------------------- the three passes
@pytest.mark.parametrize('gs', [1.0, 0.37])
def test_squared_norms(bucket, plan, gs):
    from poisson_cnn_amd import ops
    buf, g = guarded(bucket)
    before = buf.clone()
    sq = ops.grad_sqnorms(g, plan, gs).double().cpu().numpy()
    total = float(plan.total.cpu())
    ref = T.sqnorms(bucket, gs)
    for v, n in enumerate(T.SIZES):
        err, bound = abs(sq[v] - ref[v]), T.sqnorm_rel_bound(n) * ref[v]
        print('var %2d (%4d floats): err %.3g bound %.3g' % (v, n, err, bound))
        assert err <= bound, (v, n)
    assert sq[T.ZERO_VAR] == 0.0
    err, bound = abs(total - ref.sum()), T.total_rel_bound(T.SIZES) * ref.sum()
    print('total: err %.3g bound %.3g' % (err, bound))
    assert err <= bound
    assert same_bits(buf, before)                                    # the pass reads only


def test_scales(bucket, plan):
    from poisson_cnn_amd import ops
    _, g = guarded(bucket)
    ops.grad_sqnorms(g, plan, 1.0)
    sc = ops.grad_clip_scales(plan, 'clipnorm', C).cpu().numpy()
    assert sc.dtype == np.float32 and sc[T.ZERO_VAR] == 1.0 and sc[T.SMALL_VAR] == 1.0            # exactly 1.0f
    ref = T.scales(bucket, C)
    for v, n in enumerate(T.SIZES):
        err, bound = abs(float(sc[v]) - ref[v]), T.scale_rel_bound(T.sqnorm_rel_bound(n)) * ref[v]
        print('var %2d: scale %.9g ref %.9g err %.3g bound %.3g' % (v, sc[v], ref[v], err, bound))
        assert err <= bound, (v, n)
    assert sc[T.BIG_VAR] < 0.01 and sc[T.AT_C_VAR] > 1 - 1e-5


@pytest.mark.parametrize('gs', [1.0, 0.37])
def test_apply_is_scale_times_gradient_bitwise(bucket, plan, gs):
    from poisson_cnn_amd import ops
    buf, g = guarded(bucket)
    g0 = g.clone()
    ops.grad_clip_(g, plan, 'clipnorm', C, None, gs)
    sc = plan.scale.clone()
    assert same_bits(g, (g0 * f32t(gs)) * per_element(sc))
    assert guards_intact(buf)
    if gs == 1.0:                                                    # scale exactly 1: the variable keeps its bits
        off = np.concatenate([[0], np.cumsum(T.SIZES)])
        untouched = [v for v in range(len(T.SIZES)) if float(sc[v]) == 1.0]
        assert T.ZERO_VAR in untouched and T.SMALL_VAR in untouched and T.BIG_VAR not in untouched
        for v in untouched:
            assert same_bits(g[off[v]:off[v + 1]], g0[off[v]:off[v + 1]])
    # against the twin: every element within the bound its variable's scale carries, plus the two products' roundings
    ref = np.concatenate(T.clip([bucket], gs, clipnorm=C)[0])
    bound = np.concatenate([np.full(n, T.scale_rel_bound(T.sqnorm_rel_bound(n)) + 2 * T.U) for n in T.SIZES])
    assert (np.abs(g.double().cpu().numpy() - ref) <= bound * np.abs(ref)).all()


def test_clipvalue_alone_is_exact(bucket, plan):
    from poisson_cnn_amd import ops
    cv = 0.7
    buf, g = guarded(bucket)
    ops.grad_clip_(g, plan, None, 0.0, cv, 1.0)
    ref = np.concatenate(T.clip([bucket], clipvalue=cv)[0])
    assert np.array_equal(g.double().cpu().numpy(), ref) and guards_intact(buf)
    assert (np.abs(ref) == np.float32(cv)).sum() > 100 and (np.abs(ref) < np.float32(cv)).sum() > 100        # both sides of the clamp occur


def test_clipvalue_after_clipnorm(bucket, plan):
    from poisson_cnn_amd import ops
    cv = 0.05
    buf, g = guarded(bucket)
    g0 = g.clone()
    ops.grad_clip_(g, plan, 'clipnorm', C, cv, 1.0)
    normed = (g0 * f32t(1.0)) * per_element(plan.scale)
    assert same_bits(g, torch.clamp(normed, -cv, cv)) and guards_intact(buf)       # the clamp acts on the norm-clipped value: exact
    got = g.double().cpu().numpy()
    unclamped = np.concatenate(T.clip([bucket], clipnorm=C)[0])
    ref = np.concatenate(T.clip([bucket], clipnorm=C, clipvalue=cv)[0])
    rel = np.concatenate([np.full(n, T.scale_rel_bound(T.sqnorm_rel_bound(n)) + 2 * T.U) for n in T.SIZES])
    assert (np.abs(got - ref) <= rel * np.abs(ref)).all()
    sat = np.abs(unclamped) > np.float32(cv) * (1 + rel)            # clearly beyond the clamp: exactly +-cv, as in the twin
    assert sat.sum() > 100 and np.array_equal(got[sat], ref[sat])
    wrong = np.concatenate(T.clip([bucket], clipnorm=C, clipvalue=cv, variant='clipvalue_first')[0])
    assert not (np.abs(got - wrong) <= rel * np.abs(wrong)).all()


def test_determinism(bucket, plan):
    from poisson_cnn_amd import ops
    outs = []
    for _ in range(2):
        _, g = guarded(bucket)
        ops.grad_clip_(g, plan, 'clipnorm', C, 0.05, 0.37)
        outs.append((g.clone(), plan.sqnorm.clone(), plan.scale.clone(), plan.total.clone()))
    assert all(same_bits(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and torch.equal(outs[0][3], outs[1][3])


# ---------------------------------------------------------------------------------------------------------------- through the optimizers
def test_global_clipnorm_over_two_stores(bucket):
    from poisson_cnn_amd.train import SGD
    two = [bucket, T.make_bucket(C, seed=1)]
    G = T.global_norm(two)
    c = float(np.float32(0.5 * G))
    stores = [make_store(b, 100 + k) for k, b in enumerate(two)]
    g0 = [s.flat_g.clone() for s in stores]
    w0 = [s.flat_w.clone() for s in stores]
    opt = SGD(learning_rate=0.0, global_clipnorm=c)
    opt.bind(stores)
    opt.apply_gradients()
    scale = opt._global_scale.clone()
    sq_rel = T.total_rel_bound(T.SIZES * 2)
    got_norm = float(opt.global_norm)
    print('global norm %.9g ref %.9g, scale %.9g ref %.9g' % (got_norm, G, float(scale), c / G))
    assert abs(got_norm - G) <= (T.scale_rel_bound(sq_rel) + T.U) * G               # sqrt halves the relative error; one fp32 rounding
    assert abs(float(scale) - c / G) <= T.scale_rel_bound(sq_rel) * c / G
    for s, g, w in zip(stores, g0, w0):
        assert same_bits(s.flat_g, (g * f32t(1.0)) * scale)                           # ONE scale for both buckets
        assert same_bits(s.flat_w, w)                                                  # lr = 0
    # a norm below c: nothing moves
    stores = [make_store(b, 100 + k) for k, b in enumerate(two)]
    opt = SGD(learning_rate=0.0, global_clipnorm=float(np.float32(2 * G)))
    opt.bind(stores)
    opt.apply_gradients()
    assert float(opt._global_scale) == 1.0 and all(same_bits(s.flat_g, g) for s, g in zip(stores, g0))


def test_global_clipnorm_nan_poisons_every_gradient(bucket):
    from poisson_cnn_amd.train import Adam
    stores = [make_store(bucket, 100), make_store(T.make_bucket(C, seed=1), 101)]
    stores[1].flat_g[1500] = float('nan')
    opt = Adam(learning_rate=1e-3, global_clipnorm=1.0, clipvalue=0.5)               # the clamp must not turn a NaN into +-clipvalue
    opt.bind(stores)
    opt.apply_gradients()
    assert np.isnan(float(opt.global_norm))
    for s in stores:
        assert bool(torch.isnan(s.flat_g).all()) and bool(torch.isnan(s.flat_w).all())     # what TerminateOnNaN then sees in the next loss


def _optimizers():
    from poisson_cnn_amd.train import SGD, Adam
    return {'adam': lambda **kw: Adam(learning_rate=1e-2, **kw), 'amsgrad': lambda **kw: Adam(learning_rate=1e-2, amsgrad=True, **kw),
            'sgd': lambda **kw: SGD(learning_rate=1e-2, **kw), 'nesterov': lambda **kw: SGD(learning_rate=1e-2, momentum=0.9, nesterov=True, **kw)}


@pytest.mark.parametrize('kind', ['adam', 'amsgrad', 'sgd', 'nesterov'])
def test_update_kinds(kind, plan):
    from poisson_cnn_amd import ops
    make = _optimizers()[kind]
    grads = [T.make_bucket(C, seed=10 + k) for k in range(3)]

    def run(opt, preclip=None):
        store = make_store(grads[0], 7)
        opt.bind(store)
        for gv in grads:
            store.flat_g.copy_(torch.from_numpy(np.concatenate(gv)))
            if preclip is not None:
                ops.grad_clip_(store.flat_g, plan, 'clipnorm', preclip, None, 1.0)
            opt.apply_gradients()
        return store.flat_w

    plain = run(make())
    assert same_bits(run(make(clipnorm=1e30)), plain)                                # a clip that never binds changes no bit
    clipped = run(make(clipnorm=C))
    assert not same_bits(clipped, plain)
    assert same_bits(clipped, run(make(), preclip=C))                                # = the plain optimizer fed the clipped gradient


def test_decay_three_sgd_steps(bucket):
    from poisson_cnn_amd.train import SGD
    lr, d = 0.1, 0.3
    store = make_store(bucket, 9)
    g = store.flat_g.clone()
    w = store.flat_w.clone()
    opt = SGD(learning_rate=lr, decay=d)
    opt.bind(store)
    for t in range(3):
        opt.apply_gradients()
        w = w - f32t(T.decayed_lr(lr, d, t)) * g                                     # lr_t as float32 of the formula
        assert same_bits(store.flat_w, w), t
    assert opt.learning_rate == lr and opt.iterations == 3 and same_bits(store.flat_g, g)


# ---------------------------------------------------------------------------------------------------------------- a whole model step
def test_whole_model_step_with_global_clipnorm():
    """hpnn_tiny as in tests/test_gpu_model.py.  train_step is _local_step (forward, loss, backward) + _finish_step (clip, update, logs): the norm of
    the gradient is measured between the two, the clip set to half of it."""
    from poisson_cnn_amd import configs
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.train import Adam, store_variable_sizes
    from tests.test_gpu_model import build, make_inputs
    full = configs.hpnn_tiny()
    cfg = full['model']
    cfg['postsmoother_iterations'] = 1
    lossp = dict(full['training']['loss_parameters'])
    model, _ = build(cfg, 21)
    rhs, dx = make_inputs(3, 44, 38, 23)
    target = np.random.default_rng(3).standard_normal(rhs.shape).astype(np.float32) * 0.1
    loss = loss_wrapper(global_batch_size=3, **lossp)
    model.compile(loss=loss, optimizer=Adam(learning_rate=1e-3))
    assert 'grad_norm' not in model.train_step(((rhs, dx), target))                   # no clip option: the logs are what they were
    lv, mse = model._local_step(((rhs, dx), target))
    S = model.store
    g0, w0 = S.flat_g.clone(), S.flat_w.clone()
    G = float(np.linalg.norm(g0.double().cpu().numpy()))
    assert np.isfinite(G) and G > 0
    model.compile(loss=loss, optimizer=Adam(learning_rate=1e-3, global_clipnorm=0.5 * G))
    logs = model._finish_step(lv, mse)
    sizes = store_variable_sizes(S)
    rel = T.scale_rel_bound(T.total_rel_bound(sizes)) + T.U
    print('grad_norm %.9g, norm of flat_g %.9g, bound %.3g' % (float(logs['grad_norm']), G, rel * G))
    assert abs(float(logs['grad_norm']) - G) <= rel * G
    scale = model.optimizer._global_scale.clone()
    assert abs(float(scale) - 0.5) < 1e-6
    ref_store = types.SimpleNamespace(flat_w=w0.clone(), flat_g=(g0 * f32t(1.0)) * scale, specs=S.specs)
    ref_opt = Adam(learning_rate=1e-3)
    ref_opt.bind(ref_store)
    ref_opt.apply_gradients()
    assert same_bits(S.flat_w, ref_store.flat_w) and not same_bits(S.flat_w, w0)
    assert same_bits(S.flat_g, ref_store.flat_g)
