"""model.predict / evaluate / test_step, fit(validation_data=...) and EarlyStopping on the GPU, with the tiny Homogeneous_Poisson_NN_Legacy of
tests/test_gpu_model.py (and a tiny Dirichlet_BC_NN_Legacy_2 for the models without a right-hand side)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import hpnn as ohpnn, dbcnn as odb
from poisson_cnn_amd import configs
from tests import error_stats_twin as TW

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
SUM_TOL = 40 * EPS          # the kernel's sums against fp64 (tests/test_gpu_error_stats.py derives it); a ratio of two sums: twice that
LOSS_TOL = 2e-5             # the project's bound for the loss scalar
SHAPES = [(36, 40), (40, 36)]


def _r2_tol(pred, rhs, dx2, ref):
    """Bound on |sum r^2 (fp32 kernel) - sum r^2 (fp64 twin)| per sample for a prediction whose residual CANCELS (a smoothed solution: r is small
    against the terms of the Laplacian, unlike the independent random fields of tests/test_gpu_error_stats.py).  Each r carries the absolute
    error d of that file's per-point bound, so the sum moves by at most sum(2 |r| d + d^2) <= 2 d sqrt(n sum r^2) + n d^2 (Cauchy-Schwarz over the
    n interior points), plus the addition chain's SUM_TOL sum r^2."""
    N = pred.shape[0]
    n = (pred.shape[-2] - 2) * (pred.shape[-1] - 2)
    d = 8 * EPS * 4 * np.abs(pred).reshape(N, -1).max(1) * (1.0 / dx2.astype(np.float64) ** 2).sum(1) + EPS * np.abs(rhs).reshape(N, -1).max(1)
    return 2 * d * np.sqrt(n * ref[:, 5]) + n * d * d + SUM_TOL * ref[:, 5]


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _batch(H, W, seed, n=2):
    rng = np.random.default_rng(seed)
    rhs = rng.uniform(-1, 1, (n, 1, H, W))
    rhs /= np.abs(rhs).max(axis=(1, 2, 3), keepdims=True)
    return [_f32(rhs), _f32(rng.uniform(5e-3, 5e-2, (n, 1)))], _f32(rng.standard_normal((n, 1, H, W)) * 0.1)


class _Seq:
    """A Sequence-style dataset over given batches (the grid shape changes from batch to batch)."""

    def __init__(self, batches):
        self.batches = list(batches)

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.batches[i]


def _model(bn_training=False, seed=5, lr=1e-4):
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.train import Adam
    full = configs.hpnn_tiny()
    cfg = full['model']
    cfg['postsmoother_iterations'] = 2
    model = Homogeneous_Poisson_NN_Legacy(**cfg, batchnorm_training=bn_training)
    model.set_weights(ohpnn.init_params(cfg, seed=seed, gain=1.6, randomize_all=True))
    model.compile(loss=loss_wrapper(global_batch_size=2, **full['training']['loss_parameters']), optimizer=Adam(learning_rate=lr))
    return model


def _state(model):
    opt = model.optimizer
    out = [opt.iterations]
    for st, m, v in zip(model.stores, opt.ms, opt.vs):
        out += [st.flat_w.clone(), st.flat_g.clone(), st.flat_stats.clone(), m.clone(), v.clone()]
    return out


def _same_state(a, b):
    return a[0] == b[0] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[1:], b[1:]))


def test_predict_list_batches_and_sequence():
    model = _model()
    (rhs, dx), _ = _batch(*SHAPES[0], seed=1)
    want = model([rhs, dx]).cpu().numpy()
    got = model.predict([rhs, dx])
    assert isinstance(got, np.ndarray) and got.shape == (2, 1) + SHAPES[0] and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    cut = model.predict([rhs, dx], batch_size=1)
    assert cut.shape == want.shape
    for i in range(2):                                        # every chunk is the model's own answer for that sample
        one = model([rhs[i:i + 1], dx[i:i + 1]]).cpu().numpy()
        assert np.array_equal(cut[i:i + 1].view(np.uint32), one.view(np.uint32))
    assert np.linalg.norm(cut - want) <= 2e-5 * np.linalg.norm(want)          # batches of 1 and of 2: each within the project's 1e-5 of the oracle
    assert model.predict([rhs, dx], batch_size=1, steps=1).shape[0] == 1
    seq = _Seq([_batch(H, W, seed=10 + k) for k, (H, W) in enumerate(SHAPES)])
    out = model.predict(seq)                                  # two grid shapes: a list of per-batch arrays; the targets are ignored
    assert isinstance(out, list) and [o.shape for o in out] == [(2, 1) + s for s in SHAPES]
    assert np.array_equal(out[1], model(seq[1][0]).cpu().numpy())
    # return_stats: the residual columns, no ground truth needed
    p, res = model.predict([rhs, dx], return_stats=True)
    ref = TW.error_stats(p, None, rhs, np.repeat(dx, 2, axis=1))
    assert res.shape == (2, 3) and np.all(np.abs(res[:, 2] - ref[:, 7]) <= SUM_TOL * ref[:, 7])
    assert np.all(np.abs(res[:, 0] - ref[:, 5]) <= _r2_tol(p, rhs, np.repeat(dx, 2, axis=1), ref))
    with pytest.raises(NotImplementedError):
        model.evaluate([rhs, dx], p, sample_weight=np.ones(2))
    with pytest.raises(NotImplementedError):
        model.fit(seq, validation_split=0.2)


def _hand_evaluation(model, seq):
    """evaluate()'s figures from predict()'s output: the compiled loss per batch and the fp64 twin."""
    preds = model.predict(seq)
    loss_n, rows, hw, max_e, r2_tol = 0.0, [], [], 0.0, []
    for ((rhs, dx), y), p in zip(seq.batches, preds):
        dev = lambda a: torch.from_numpy(a).cuda()
        loss_n += float(model.loss_fn.value(dev(y), dev(p), dev(rhs), dev(np.repeat(dx, 2, axis=1)))) * 2       # global_batch_size = 2
        rows.append(TW.error_stats(p, y, rhs, np.repeat(dx, 2, axis=1)))
        r2_tol.append(_r2_tol(p, rhs, np.repeat(dx, 2, axis=1), rows[-1]))
        hw += [p.shape[2] * p.shape[3]] * p.shape[0]
        max_e = max(max_e, float(np.abs(p - y).max()))                                                          # float32, as the kernel forms it
    s, hw = np.concatenate(rows), np.asarray(hw, dtype=np.float64)
    return {'loss': loss_n / len(s), 'mse': s[:, 1].sum() / hw.sum(), 'mae': s[:, 0].sum() / hw.sum(), 'rel_l2': np.sqrt(s[:, 1] / s[:, 3]).mean(),
            'mae_over_peak': (s[:, 0] / hw / s[:, 4]).mean(), 'max_abs_error': max_e, 'rel_residual': np.sqrt(s[:, 5] / s[:, 7]).mean()}, s, np.concatenate(r2_tol)


@pytest.mark.parametrize('bn_training', [False, True])
def test_evaluate_matches_hand_aggregation_and_leaves_the_state_alone(bn_training):
    model = _model(bn_training=bn_training)
    seq = _Seq([_batch(H, W, seed=20 + k) for k, (H, W) in enumerate(SHAPES)])
    model.train_step((tuple(seq[0][0]), seq[0][1]))           # gradients, Adam moments and a step count that are not zero
    before = _state(model)
    res = model.evaluate(seq, return_dict=True, per_sample=True)
    pair = model.evaluate(seq)
    one = model.test_step(seq[0])
    model.predict(seq, return_stats=True)
    assert _same_state(before, _state(model))
    want, rows, r2_tol = _hand_evaluation(model, seq)
    assert _same_state(before, _state(model))
    for k, v in want.items():
        print('%s: evaluate %.9g, by hand %.9g' % (k, res[k], v))
    assert abs(res['loss'] - want['loss']) <= LOSS_TOL * abs(want['loss'])
    for k in ('mse', 'mae'):
        assert abs(res[k] - want[k]) <= SUM_TOL * want[k], k
    for k in ('rel_l2', 'mae_over_peak'):
        assert abs(res[k] - want[k]) <= 2 * SUM_TOL * want[k], k
    # sqrt(sum r^2 / sum f^2): half the relative error of each sum, to first order (doubled here for the second order)
    rr_tol = (np.sqrt(rows[:, 5] / rows[:, 7]) * (r2_tol / rows[:, 5] + SUM_TOL)).mean()
    print('rel_residual: error %.3g, bound %.3g' % (abs(res['rel_residual'] - want['rel_residual']), rr_tol))
    assert abs(res['rel_residual'] - want['rel_residual']) <= rr_tol
    assert res['max_abs_error'] == want['max_abs_error']
    assert res['skipped_rel_l2'] == 0 and res['skipped_rel_residual'] == 0 and res['samples'] == 4
    assert pair == [res['loss'], res['mse']]
    assert res['stats'].shape == (4, 8) and list(res['H']) == [36, 36, 40, 40] and list(res['W']) == [40, 40, 36, 36]
    sums = [0, 1, 3, 7]
    assert np.all(np.abs(res['stats'][:, sums] - rows[:, sums]) <= SUM_TOL * rows[:, sums])
    assert np.all(np.abs(res['stats'][:, 5] - rows[:, 5]) <= r2_tol)
    assert set(one) >= {'loss', 'mse', 'stats'} and np.array_equal(one['stats'].cpu().numpy().astype(np.float64), res['stats'][:2])
    # the list form, cut into batches, is the same evaluation
    (rhs, dx), y = seq[0]
    a = model.evaluate([rhs, dx], y, batch_size=1, return_dict=True)
    b = model.evaluate(_Seq([seq[0]]), return_dict=True)
    # (two forwards of the same sample in batches of 1 and 2 are each within the project's 1e-5 of the oracle, not bit-equal to each other)
    assert a['samples'] == b['samples'] == 2 and abs(a['mse'] - b['mse']) <= 1e-4 * b['mse'] and abs(a['max_abs_error'] - b['max_abs_error']) <= 1e-4 * b['max_abs_error']
    assert model.eval_sync is None                            # no DataParallel attached: no collective


class _Record:
    def __init__(self):
        self.epochs = []

    def set_model(self, model):
        self.model = model

    def on_batch_end(self, batch, logs):
        pass

    def on_epoch_end(self, epoch, logs):
        self.epochs.append(dict(logs))


def test_fit_with_validation_checkpoint_and_early_stopping(tmp_path):
    from poisson_cnn_amd.train import EarlyStopping, ModelCheckpoint, ReduceLROnPlateau
    model = _model()
    train = _Seq([_batch(H, W, seed=30 + k) for k, (H, W) in enumerate(SHAPES)])
    val = _Seq([_batch(H, W, seed=40 + k) for k, (H, W) in enumerate(SHAPES)])
    # today's history without validation data
    hist = model.fit(train, epochs=1, verbose=0)
    assert list(hist) == ['loss', 'mse', 'lr', 'loss_epoch_mean', 'mse_epoch_mean'] and all(len(v) == 1 for v in hist.values())
    # validation: val_* in the history and in what the callbacks see, before they run
    rec = _Record()
    path = str(tmp_path / 'best')
    plateau = ReduceLROnPlateau(monitor='val_loss', patience=100)
    hist = model.fit(train, epochs=2, verbose=0, validation_data=val, callbacks=[rec, ModelCheckpoint(path, monitor='val_loss'), plateau])
    vals = ['val_loss', 'val_mse', 'val_rel_l2', 'val_rel_residual']
    assert list(hist) == ['loss', 'mse', 'lr', 'loss_epoch_mean', 'mse_epoch_mean'] + vals
    assert all(len(hist[k]) == 2 and all(math.isfinite(x) and x > 0 for x in hist[k]) for k in vals)
    assert len(rec.epochs) == 2 and [e['val_loss'] for e in rec.epochs] == hist['val_loss'] and set(rec.epochs[0]) == set(hist)
    assert os.path.exists(path + '.npz') and plateau.best in hist['val_loss']      # both callbacks found their monitor
    ev = model.evaluate(val, return_dict=True)                # the last epoch's validation ran on the weights the model has now
    assert ev['loss'] == hist['val_loss'][-1] and ev['mse'] == hist['val_mse'][-1]
    # the tuple form and validation_freq: only every second epoch has the figures
    (rhs, dx), y = val[0]
    hist = model.fit(train, epochs=2, verbose=0, validation_data=([rhs, dx], y), validation_freq=2, validation_batch_size=1)
    assert len(hist['val_loss']) == 1 and len(hist['loss']) == 2
    # EarlyStopping: after the first epoch the validation targets turn into noise with a peak of ~4e-5.  The loss divides each sample's error
    # by its target's peak (scale_sample_loss_by_target_peak_magnitude), so it grows by four orders of magnitude, which two training steps at
    # this learning rate cannot make up: the second epoch cannot improve and is the last
    class _Spoil(_Record):
        def on_epoch_end(self, epoch, logs):
            if epoch == 0:
                val.batches = [(inp, _f32(np.random.default_rng(50 + k).standard_normal(y.shape) * 1e-5)) for k, (inp, y) in enumerate(val.batches)]
    stop = EarlyStopping(patience=0, restore_best_weights=True)
    kept = []

    class _Keep(_Record):
        def on_epoch_end(self, epoch, logs):
            kept.append([st.flat_w.clone() for st in self.model.stores])
    hist = model.fit(train, epochs=5, verbose=0, validation_data=val, callbacks=[_Keep(), stop, _Spoil()])
    assert len(hist['loss']) == 2 and stop.stopped_epoch == 1 and model.stop_training and hist['val_loss'][1] > hist['val_loss'][0]
    assert all(torch.equal(st.flat_w, w) for st, w in zip(model.stores, kept[0]))           # the first epoch's weights are back
    assert not all(torch.equal(a, b) for a, b in zip(kept[0], kept[1]))


def test_boundary_model_evaluates_without_a_right_hand_side():
    from poisson_cnn_amd.models import Dirichlet_BC_NN_Legacy_2
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.train import Adam
    full = configs.dbcnn_tiny()
    cfg = full['model']
    model = Dirichlet_BC_NN_Legacy_2(**cfg)
    model.set_weights(odb.init_params(cfg, seed=3, gain=1.5, randomize_all=True))
    model.compile(loss=loss_wrapper(global_batch_size=2, **full['training']['loss_parameters']), optimizer=Adam(learning_rate=1e-4))
    rng = np.random.default_rng(7)
    bc = _f32(np.cumsum(rng.standard_normal((2, 1, 40)), axis=2) * 0.2)
    dx = _f32(rng.uniform(5e-3, 5e-2, (2, 1)))
    y = _f32(rng.standard_normal((2, 1, 36, 40)) * 0.3)
    before = _state(model)
    res = model.evaluate([bc, dx], y, return_dict=True, per_sample=True)
    pred = model.predict([bc, dx, 36])
    assert _same_state(before, _state(model))
    assert pred.shape == (2, 1, 36, 40) and np.array_equal(pred, model([bc, dx, 36]).cpu().numpy())
    ref = TW.error_stats(pred, y)
    sums = [0, 1, 3]
    assert np.all(np.abs(res['stats'][:, sums] - ref[:, sums]) <= SUM_TOL * ref[:, sums])
    assert np.array_equal(res['stats'][:, [2, 4]], np.stack([np.abs(pred - y).reshape(2, -1).max(1), np.abs(y).reshape(2, -1).max(1)], 1).astype(np.float64))
    assert np.all(res['stats'][:, 5:] == 0.0)                 # no right-hand side among the inputs: no residual
    assert math.isnan(res['rel_residual']) and res['skipped_rel_residual'] == 2 and res['skipped_rel_l2'] == 0
    assert math.isfinite(res['loss']) and abs(res['mse'] - ref[:, 1].sum() / (2 * 36 * 40)) <= SUM_TOL * res['mse']
    with pytest.raises(ValueError):
        model.predict([bc, dx])                               # neither a target nor an x_output_resolution
