"""No GPU: the clip plan through the C-ABI, the optimizers' argument checks, the decay schedule, and a check that the fp64 twin
(tests/grad_clip_twin.py) tells the TF semantics from two wrong variants by far more than the bound the GPU tests allow."""
import numpy as np
import pytest

from poisson_cnn_amd import configs, ops
from poisson_cnn_amd.train import SGD, Adam, choose_optimizer, store_variable_sizes
from tests import grad_clip_twin as T


def _hpnn_store():
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    return Homogeneous_Poisson_NN_Legacy(device='cpu', **configs.hpnn()['model']).store


@pytest.fixture(scope='module')
def hpnn_store():
    return _hpnn_store()


def _check_plan(sizes):
    plan = ops.grad_clip_plan(sizes)
    sizes = np.asarray(sizes, np.int64)
    assert plan.n_vars == len(sizes) and plan.numel == sizes.sum()
    assert plan.n_items == sum(-(-int(n) // T.CHUNK) for n in sizes) == len(plan.item_var)
    assert (plan.item_len >= 1).all() and (plan.item_len <= T.CHUNK).all()                    # no item longer than the chunk
    assert (np.diff(plan.item_var) >= 0).all()                                                 # variable ids are monotone
    off = np.concatenate([[0], np.cumsum(sizes)])
    v = plan.item_var
    assert (plan.item_start >= off[v]).all() and (plan.item_start + plan.item_len <= off[v + 1]).all()   # no item crosses a variable boundary
    covered = np.zeros(plan.numel, np.int32)
    for s, n in zip(plan.item_start, plan.item_len):
        covered[s:s + n] += 1
    assert (covered == 1).all()                                                                # every float exactly once
    assert (plan.item_start[1:] == plan.item_start[:-1] + plan.item_len[:-1]).all()            # in physical order, no gaps
    assert plan.var_first_item[0] == 0 and plan.var_first_item[-1] == plan.n_items
    for k in range(len(sizes)):
        assert (v[plan.var_first_item[k]:plan.var_first_item[k + 1]] == k).all()
    assert plan.workspace_bytes >= 4 * plan.n_items + 8 * plan.n_vars and plan.workspace_bytes % 8 == 0
    return plan


def test_plan_tiles_the_test_sizes():
    plan = _check_plan(T.SIZES)
    assert plan.n_items == len(T.SIZES) + 1                     # 4099 floats: 4096 + 3
    assert list(plan.item_len[-2:]) == [4096, 3]
    assert plan.item_start[1] % 4 == 1 and plan.item_start[2] % 4 == 0 and plan.item_start[4] % 4 == 1      # misaligned starts are exercised


def test_plan_tiles_the_hpnn_bucket(hpnn_store):
    S = hpnn_store
    sizes = store_variable_sizes(S)
    assert sum(sizes) == S.n_trainable and len(sizes) == len(S.trainable_names())
    # the physical order of flat_g: every trainable view of the store sits where the cumulative sizes say
    off = np.concatenate([[0], np.cumsum(sizes)])
    where = sorted((S.g[n].storage_offset(), S.g[n].numel()) for n in S.trainable_names())
    assert where == [(int(off[i]), int(sizes[i])) for i in range(len(sizes))]
    plan = _check_plan(sizes)
    assert max(sizes) > T.CHUNK and plan.n_items > plan.n_vars


def test_plan_rejects_bad_sizes_and_takes_empty_variables():
    with pytest.raises(ValueError):
        ops.grad_clip_plan([4, -1])
    plan = _check_plan([0, 7, 0])
    assert plan.n_items == 1 and list(plan.var_first_item) == [0, 0, 1, 1]


@pytest.mark.parametrize('cls', [Adam, SGD])
def test_argument_checks(cls):
    with pytest.raises(ValueError, match='both'):
        cls(clipnorm=1.0, global_clipnorm=1.0)
    for k in ('clipnorm', 'global_clipnorm', 'clipvalue', 'decay'):
        with pytest.raises(ValueError, match=k):
            cls(**{k: -1e-3})
    with pytest.raises(NotImplementedError, match='gradient_transformers'):
        cls(gradient_transformers=[])
    with pytest.raises(NotImplementedError):
        cls(clipnorm=1.0, centered=True)
    assert cls(lr=0.25).learning_rate == 0.25                   # the Keras alias
    o = cls(clipnorm=None, clipvalue=None, global_clipnorm=None, decay=0.0)       # what a JSON that spells out the Keras defaults passes
    assert not o.clips and o.decay == 0.0 and o.decayed_learning_rate(5) == o.learning_rate


def test_the_four_options_construct():
    """Each of these raised NotImplementedError before the options existed."""
    a = Adam(clipnorm=1.0)
    assert (a.clip_mode, a.clipnorm, a.clips) == ('clipnorm', 1.0, True)
    s = SGD(global_clipnorm=2.0)
    assert (s.clip_mode, s.global_clipnorm, s.clips) == ('global_clipnorm', 2.0, True)
    v = Adam(clipvalue=0.5)
    assert (v.clip_mode, v.clipvalue, v.clips) == (None, 0.5, True)
    d = Adam(decay=1e-3)
    assert d.decay == 1e-3 and not d.clips
    o = choose_optimizer('sgd')(learning_rate=0.1, momentum=0.9, nesterov=True, clipnorm=3.0, clipvalue=1.0, decay=0.5)
    assert (o.clipnorm, o.clipvalue, o.decay, o.momentum, o.nesterov) == (3.0, 1.0, 0.5, 0.9, True)


@pytest.mark.parametrize('cls', [Adam, SGD])
def test_decay_schedule(cls):
    o = cls(learning_rate=0.02, decay=0.3)
    for t in range(4):
        assert o.decayed_learning_rate(t) == T.decayed_lr(0.02, 0.3, t) == 0.02 / (1 + 0.3 * t)
    assert o.decayed_learning_rate() == 0.02                    # t = 0 on the first step
    o.iterations = 3
    assert o.decayed_learning_rate() == 0.02 / (1 + 0.3 * 3)
    o.learning_rate = 0.01                                       # what ReduceLROnPlateau does: the base value moves, the schedule follows
    assert o.decayed_learning_rate() == 0.01 / (1 + 0.3 * 3) and o.learning_rate == 0.01


def test_twin_tells_the_wrong_variants_apart():
    """The GPU tests compare bitwise or within ~1e-6 relative; the wrong variants are off by tens of percent on the same bucket."""
    c = 1.0
    g = T.make_bucket(c)
    ref = np.concatenate(T.clip([g], clipnorm=c)[0])
    wrong = np.concatenate(T.clip([g], clipnorm=c, variant='global_for_per_variable')[0])
    bound = max(T.scale_rel_bound(T.sqnorm_rel_bound(n)) for n in T.SIZES)
    assert bound < 1e-5
    assert np.linalg.norm(wrong - ref) > 0.1 * np.linalg.norm(ref) > 1e4 * bound * np.linalg.norm(ref)
    # the per-variable semantics: untouched below c, norm c above it
    out = T.clip([g], clipnorm=c)[0]
    assert np.array_equal(out[T.SMALL_VAR], g[T.SMALL_VAR].astype(np.float64)) and not out[T.ZERO_VAR].any()
    assert abs(np.linalg.norm(out[T.BIG_VAR]) - c) < 1e-12
    ref2 = np.concatenate(T.clip([g], clipnorm=c, clipvalue=0.05)[0])
    wrong2 = np.concatenate(T.clip([g], clipnorm=c, clipvalue=0.05, variant='clipvalue_first')[0])
    assert np.abs(ref2).max() <= np.float32(0.05) and np.linalg.norm(wrong2 - ref2) > 0.1 * np.linalg.norm(ref2)
    # global: one scale for everything, NaN everywhere when the norm is not finite
    two = [g, T.make_bucket(c, seed=1)]
    G = T.global_norm(two)
    out = T.clip(two, global_clipnorm=0.5 * G)
    assert np.allclose(np.concatenate(out[0]), 0.5 * np.concatenate(g)) and abs(T.global_norm(out) - 0.5 * G) < 2 * T.U * G      # c reaches the library as fp32
    bad = [[v.copy() for v in g], two[1]]
    bad[0][4][7] = np.nan
    assert all(np.isnan(v).all() for b in T.clip(bad, global_clipnorm=1.0) for v in b)


def test_bound_is_derived_from_the_plan():
    assert T.item_lengths(4099) == [4096, 3] and T.item_lengths(1) == [1]
    # 4096 floats: 16 + 2 lane terms, 6 + 2 tree levels, 2 roundings per term
    assert abs(T.sqnorm_rel_bound(4096) - T.gamma(28)) < 3 * T.U
    assert T.sqnorm_rel_bound(1) < T.sqnorm_rel_bound(1025) < T.sqnorm_rel_bound(4099) < 40 * T.U
