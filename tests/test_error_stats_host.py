"""Host-side checks (no GPU) of the evaluation feature: the fp64 twin of pcnn_error_stats itself, EarlyStopping's decisions, evaluate()'s
aggregation of per-batch statistics and the data-parallel combine over two gloo ranks."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import error_stats_twin as TW


# ------------------------------------------------------------------------------------------------ the twin
def test_twin_quadratic_has_zero_residual():
    """p = x^2 + y^2 on a grid with dx != dy: the second differences are exactly 2 per axis, so with rhs = 4 the residual vanishes to fp64
    rounding and sum f^2 = 16 (H-2)(W-2)."""
    H, W, dx0, dx1 = 9, 12, 0.03, 0.0125
    y, x = np.meshgrid(np.arange(H) * dx0, np.arange(W) * dx1, indexing='ij')
    p = (x ** 2 + y ** 2)[None]
    s = TW.error_stats(p, target=p, rhs=np.full_like(p, 4.0), dx=np.array([[dx0, dx1]]))
    assert s.shape == (1, 8)
    assert s[0, 6] < 1e-9 and s[0, 5] < 1e-18 * (H - 2) * (W - 2)                 # |r| at rounding level: terms of size p/dx^2 ~ 1e3 in fp64
    assert s[0, 7] == 16.0 * (H - 2) * (W - 2)
    assert np.all(s[0, :3] == 0.0) and abs(s[0, 3] - (p ** 2).sum()) < 1e-12 * (p ** 2).sum() and s[0, 4] == p.max()
    # swapping the two spacings breaks it: column 0 of dx belongs to the H axis
    assert TW.error_stats(p, rhs=np.full_like(p, 4.0), dx=np.array([[dx1, dx0]]))[0, 6] > 1.0


def test_twin_by_hand_on_3x3():
    p = np.array([[[1., 2., 3.], [4., 5., 7.], [8., 6., 9.]]])
    t = np.array([[[1., 0., 3.], [4., 3., 7.], [8., 6., -12.]]])
    f = np.full((1, 3, 3), 100.0)
    f[0, 1, 1] = 0.5
    dx = np.array([[0.5, 0.25]])
    s = TW.error_stats(p, t, f, dx)
    # e = 2 at (0,1), 2 at (1,1), 21 at (2,2)
    assert s[0, 0] == 25.0 and s[0, 1] == 4.0 + 4.0 + 441.0 and s[0, 2] == 21.0
    assert s[0, 3] == 1 + 9 + 16 + 9 + 49 + 64 + 36 + 144 and s[0, 4] == 12.0
    r = (2.0 - 10.0 + 6.0) / 0.25 + (4.0 - 10.0 + 7.0) / 0.0625 - 0.5             # the one interior point: -8 + 16 - 0.5
    assert r == 7.5 and s[0, 5] == r * r and s[0, 6] == abs(r) and s[0, 7] == 0.25
    # NULL handling of the twin, and the (N,1,H,W) / (N,H,W,1) layouts
    assert np.all(TW.error_stats(p, None, f, dx)[0, :5] == 0.0) and np.all(TW.error_stats(p, t)[0, 5:] == 0.0)
    assert np.array_equal(TW.error_stats(p[:, None], t[:, None], f[:, None], dx), s) and np.array_equal(TW.error_stats(p[..., None], t, f, dx), s)
    with pytest.raises(ValueError):
        TW.error_stats(p[:, :2], None, f[:, :2], dx)


# ------------------------------------------------------------------------------------------------ EarlyStopping
class _M:
    stop_training = False


def _run(cb, values, key='val_loss'):
    """-> index of the epoch after which training stopped (None: never)."""
    m = _M()
    m.stop_training = False
    cb.set_model(m)
    for e, v in enumerate(values):
        cb.on_epoch_end(e, {} if v is None else {key: v})
        if m.stop_training:
            return e
    return None


def test_early_stopping_decisions():
    from poisson_cnn_amd.train import EarlyStopping
    assert _run(EarlyStopping(patience=0), [3.0, 2.0, 2.5, 1.0]) == 2                     # the first epoch that does not improve
    assert _run(EarlyStopping(patience=1), [3.0, 2.0, 2.5, 1.0]) == 2                     # (Keras: wait >= patience is checked after wait += 1)
    assert _run(EarlyStopping(patience=2), [3.0, 2.0, 2.5, 1.0, 1.5, 1.2]) == 5           # the improvement at epoch 3 resets the count
    assert _run(EarlyStopping(patience=2), [3.0, 2.0, 1.5, 1.0]) is None
    # min_delta: an improvement smaller than it does not count
    assert _run(EarlyStopping(patience=2, min_delta=0.5), [3.0, 2.8, 2.7, 1.0]) == 2
    assert _run(EarlyStopping(patience=2, min_delta=-0.5), [3.0, 2.8, 2.7, 1.0]) == 2     # Keras takes the magnitude
    # mode
    assert _run(EarlyStopping(monitor='score', mode='max', patience=1), [1.0, 2.0, 1.5], key='score') == 2
    assert _run(EarlyStopping(monitor='val_acc', patience=1), [0.1, 0.2, 0.3, 0.25], key='val_acc') == 3        # auto: 'acc' -> max
    assert _run(EarlyStopping(monitor='val_loss', mode='auto', patience=1), [1.0, 2.0]) == 1
    with pytest.raises(ValueError):
        EarlyStopping(mode='sideways')
    # baseline: the value to beat from the first epoch on
    assert _run(EarlyStopping(patience=2, baseline=1.0), [3.0, 2.0, 0.5]) == 1
    assert _run(EarlyStopping(patience=3, baseline=1.0), [3.0, 2.0, 0.5, 0.6, 0.7, 0.8]) == 5
    # an epoch without the monitored value (validation_freq > 1) neither counts nor fails
    assert _run(EarlyStopping(patience=1), [3.0, None, None, 2.0, None, 2.5]) == 5
    # a second fit() starts afresh
    cb = EarlyStopping(patience=1)
    assert _run(cb, [1.0, 2.0]) == 1 and cb.stopped_epoch == 1
    assert _run(cb, [5.0, 4.0, 4.5]) == 2


def test_early_stopping_restores_the_best_weights():
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.train import EarlyStopping

    class _Store:
        def __init__(self):
            self.flat_w, self.flat_stats = torch.zeros(4), torch.zeros(2)

    class _Model(_M):
        def __init__(self):
            self.stores = [_Store(), _Store()]
    m = _Model()
    cb = EarlyStopping(patience=2, restore_best_weights=True)
    cb.set_model(m)
    v0 = ops.filter_version()
    for e, v in enumerate([3.0, 1.0, 2.0, 2.5]):
        for k, s in enumerate(m.stores):                  # "training" moved the weights before the epoch ended
            s.flat_w.fill_(10.0 * k + e)
            s.flat_stats.fill_(-10.0 * k - e)
        cb.on_epoch_end(e, {'val_loss': v})
    assert m.stop_training and cb.stopped_epoch == 3 and cb.best == 1.0
    for k, s in enumerate(m.stores):                      # epoch 1 was the best
        assert torch.all(s.flat_w == 10.0 * k + 1) and torch.all(s.flat_stats == -10.0 * k - 1)
    assert ops.filter_version() != v0                     # cached filter spectra are stale after the restore


# ------------------------------------------------------------------------------------------------ evaluate()'s aggregation
def _rows(sum_abs_e, sum_e2, max_e, sum_t2, max_t, sum_r2, max_r, sum_f2):
    return [sum_abs_e, sum_e2, max_e, sum_t2, max_t, sum_r2, max_r, sum_f2]


def test_aggregation_from_given_batch_statistics():
    from poisson_cnn_amd import evaluation as E
    # batch A: 2 samples on 4 x 5 points, compiled loss 0.3 with global_batch_size 4; batch B: 1 sample on 2 x 3 points, loss 0.5
    A = np.array([_rows(2.0, 1.0, 0.5, 4.0, 2.0, 9.0, 1.5, 1.0),
                  _rows(4.0, 8.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.0)])          # zero target AND zero rhs: skipped in both relative means
    B = np.array([_rows(3.0, 6.0, 2.5, 24.0, 3.0, 4.0, 1.0, 16.0)])
    ta, ma = E.batch_totals(A, 4, 5, 0.3, 4)
    tb, mb = E.batch_totals(B, 2, 3, 0.5, 4)
    res = E.finish(ta + tb, max(ma, mb))
    assert res['samples'] == 3
    assert res['loss'] == pytest.approx((0.3 * 4 + 0.5 * 4) / 3, rel=1e-15)
    assert res['mse'] == pytest.approx(15.0 / 46.0, rel=1e-15) and res['mae'] == pytest.approx(9.0 / 46.0, rel=1e-15)
    assert res['rel_l2'] == pytest.approx((math.sqrt(1.0 / 4.0) + math.sqrt(6.0 / 24.0)) / 2, rel=1e-15)
    assert res['mae_over_peak'] == pytest.approx(((2.0 / 20) / 2.0 + (3.0 / 6) / 3.0) / 2, rel=1e-15)
    assert res['max_abs_error'] == 2.5
    assert res['rel_residual'] == pytest.approx((3.0 + 0.5) / 2, rel=1e-15)
    assert res['skipped_rel_l2'] == 1 and res['skipped_rel_residual'] == 1
    # global_batch_size None: the loss is a mean over the batch's own samples
    t, _ = E.batch_totals(A, 4, 5, 0.3, None)
    assert t[E.TOTALS.index('loss_n')] == pytest.approx(0.6)
    # a model without a right-hand side: residual columns all zero -> NaN, every sample skipped; nothing evaluated -> NaN, not an exception
    C = B.copy()
    C[:, 5:] = 0.0
    res = E.finish(*E.batch_totals(C, 2, 3, 0.5, 1))
    assert math.isnan(res['rel_residual']) and res['skipped_rel_residual'] == 1 and res['rel_l2'] == pytest.approx(0.5)
    assert math.isnan(E.finish(np.zeros(len(E.TOTALS)), 0.0)['loss'])


def test_input_lists_are_cut_into_batches():
    from poisson_cnn_amd import evaluation as E
    rhs, dx, y = np.arange(5 * 6).reshape(5, 1, 2, 3), np.arange(5.0).reshape(5, 1), np.arange(5 * 6).reshape(5, 1, 2, 3) * 2
    b = E.ArrayBatches([rhs, dx, 7], y, batch_size=2)
    assert len(b) == 3 and not E.is_sequence([rhs, dx]) and E.is_sequence(b) and not E.is_sequence(rhs)
    (r2, d2, X), y2 = b[2]
    assert X == 7 and np.array_equal(r2, rhs[4:]) and np.array_equal(d2, dx[4:]) and np.array_equal(y2, y[4:])
    assert len(E.ArrayBatches([rhs, dx])) == 1 and E.ArrayBatches([rhs, dx])[0][1] is None          # Keras' default of 32
    with pytest.raises(ValueError):
        E.ArrayBatches([rhs, dx[:4]])
    with pytest.raises(IndexError):
        b[3]
    with pytest.raises(NotImplementedError):
        E.reject_unsupported('fit', {'validation_split': 0.1})
    with pytest.raises(NotImplementedError):
        E.reject_unsupported('evaluate', {'sample_weight': None})
    with pytest.raises(TypeError):
        E.reject_unsupported('fit', {'no_such_argument': 1})


# ------------------------------------------------------------------------------------------------ the data-parallel combine
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batches(rank):
    rng = np.random.default_rng(40 + rank)
    out = []
    for H, W in ((4, 5), (3, 7)):
        s = rng.uniform(0.5, 2.0, (2, 8))
        out.append((s, H, W, 0.1 * (rank + 1) + 0.01 * H))
    return out


def _eval_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from poisson_cnn_amd import evaluation as E, parallel
    dp = parallel.DataParallel.from_env(backend='gloo')
    tot, worst = np.zeros(len(E.TOTALS)), 0.0
    for s, H, W, loss in _rank_batches(rank):
        t, m = E.batch_totals(s, H, W, loss, 4)
        tot, worst = tot + t, max(worst, m)
    g, gm = dp.global_eval_totals(tot, worst)
    q.put((rank, E.finish(g, gm)))
    torch.distributed.destroy_process_group()


def test_eval_totals_combine_over_two_gloo_ranks():
    from poisson_cnn_amd import evaluation as E, parallel
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0] == res[1]                                          # every rank's callbacks see the same figures
    tot, worst = np.zeros(len(E.TOTALS)), 0.0
    for rank in range(2):                                            # ... those of one process that evaluated all four batches
        for s, H, W, loss in _rank_batches(rank):
            t, m = E.batch_totals(s, H, W, loss, 4)
            tot, worst = tot + t, max(worst, m)
    want = E.finish(tot, worst)
    assert want['samples'] == 8 and res[0]['max_abs_error'] == want['max_abs_error']
    for k, v in want.items():
        assert res[0][k] == pytest.approx(v, rel=1e-14), k
    # no DataParallel attached / a single rank: no collective, the totals come back as they are
    t1, m1 = parallel.DataParallel().global_eval_totals(tot, worst)
    assert np.array_equal(t1, tot) and m1 == worst
