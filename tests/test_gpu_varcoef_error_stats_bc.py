"""pcnn_varcoef_bc_error_stats (csrc/error_stats.hip, ops.varcoef_error_stats(neumann_mask=...)) against tests/varcoef_error_stats_bc_twin.py on the
same fp32 inputs, for all 16 masks, and Homogeneous_Poisson_NN_Legacy(density_input=True, residual_metrics=True) on the tiny
model and the 2 x 24 x 28 batch of tests/test_gpu_varcoef_model.py with the edge types of tests/test_gpu_varcoef_model_bc.py.

The bound on the sums (columns 1, 3, 5, 7; 0 has no term rounding and takes the same bound), derived as tests/test_gpu_varcoef_stats.py derives its
own.  The twin forms every term (e, t, r, f) in float32 in the kernel's operation order and adds in float64; all terms of a sum are non-negative, so
the kernel's float32 sum is off by at most (longest addition chain + the roundings that make one term of those float32 values) * eps of itself.
The decomposition is that of the all-Dirichlet kernel (64 bands of rows per sample, 16 waves per band, one row per wave at a time, lanes stride
the columns by 64):
    per lane ceil(ceil(H / 64) / 16) * ceil(W / 64) additions, 6 butterfly steps over the wave's lanes, 15 additions over the band's waves,
    6 butterfly steps over the bands;  the term is one more rounding (e * e, t * t, r * r, f * f) - the weight w = 1, 1/2, 1/4 scales it exactly.
3 x 3, 3 x 4, 9 x 11 and 24 x 28: 1 + 27 additions, (28 + 1) eps;  70 x 133: two rows per band - one per wave - and three column strides,
3 + 27 additions, (30 + 1) eps.  max|r| (column 6) is one term and no sum: the bits of the float32-order twin."""
import functools
from ctypes import c_int

import numpy as np
import pytest
import torch

from tests import bc_edges_twin as E, test_gpu_varcoef_model as VM, test_gpu_varcoef_model_bc as VB, varcoef_error_stats_bc_twin as ST

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
N = 2
# 3 x 3: every unknown is an edge or a corner; 3 x 4; 9 x 11; 70 x 133: more than one row per band and ragged bands (70 = 35 bands of 2 rows, 29 empty),
# three lane strides with a ragged last one (133 = 64 + 64 + 5) - columns 0 and W - 1 sit in different strides, with an edge-free stride between
SHAPES = [(3, 3), (3, 4), (9, 11), (70, 133)]
MASKS = list(range(16))
SUMS = (0, 1, 3, 5, 7)


def chain(H, W):
    """The longest addition chain of one sum (see the module docstring)."""
    cdiv = lambda a, b: -(-a // b)
    return cdiv(cdiv(H, 64), 16) * cdiv(W, 64) + 6 + 15 + 6


def sum_tol(H, W):
    return (chain(H, W) + 1) * EPS


assert [chain(*s) for s in SHAPES] == [28, 28, 28, 30] and chain(VM.H, VM.W) == 28

bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    """(host arrays, device tensors): pred, target, rho in (1, 10), rhs independent of pred (the residual does not cancel), one dx per sample"""
    rng = np.random.default_rng(1000 * H + W)
    pred = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    target = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
    rho = rng.uniform(1.0, 10.0, (N, H, W)).astype(np.float32)
    rhs = (rng.standard_normal((N, H, W)) * 50).astype(np.float32)
    dx = np.array([0.0123, 0.0371], dtype=np.float32)
    arrs = (pred, target, rho, rhs, dx)
    return arrs, tuple(torch.from_numpy(a).cuda() for a in arrs)


@functools.lru_cache(maxsize=None)
def _errors_only(H, W):
    """ops.error_stats without a right-hand side: what columns 0..4 must be, bit for bit"""
    from poisson_cnn_amd import ops
    _, (pred, target, _, _, _) = _inputs(H, W)
    return ops.error_stats(pred, target).cpu().numpy()


def _call(mask, pred, target, rho, rhs, dx):
    from poisson_cnn_amd import ops
    return ops.varcoef_error_stats(pred, rho, target, rhs, dx, neumann_mask=mask).cpu().numpy()


def _raw(mask, H, W, pred, target, rho, rhs, dx):
    """the new C entry point itself, which ops takes only for a non-zero mask"""
    from poisson_cnn_amd import ops
    out = ops.empty((N, 8), pred.device)
    ops.handle().call('pcnn_varcoef_bc_error_stats', c_int(N), c_int(H), c_int(W), c_int(mask), ops._p(pred), ops._p(target), ops._p(rho), ops._p(rhs),
                      ops._p(dx), ops._p(out))
    return out.cpu().numpy()


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_all_masks_match_the_float32_order_twin(H, W, mask):
    (pred, target, rho, rhs, dx), dev = _inputs(H, W)
    got = _call(mask, *dev)
    ref = ST.error_stats(pred, rho, target, rhs, dx, mask, float32_terms=True)
    assert got.shape == (N, 8) and got.dtype == np.float32
    rel = np.abs(got[:, SUMS] - ref[:, SUMS]) / ref[:, SUMS]
    print('%dx%d mask %d: sums rel. error / tolerance %.3g, max|r| %r vs %r' % (H, W, mask, rel.max() / sum_tol(H, W), got[:, 6].tolist(), ref[:, 6].tolist()))
    assert np.array_equal(got[:, 6].astype(np.float64), ref[:, 6])
    assert np.all(ref[:, SUMS] > 0) and np.all(rel <= sum_tol(H, W))
    assert np.array_equal(bits(got[:, :5]), bits(_errors_only(H, W)[:, :5]))


@pytest.mark.parametrize('H,W', SHAPES)
def test_mask_0_through_the_new_entry_point_is_the_old_one(H, W):
    from poisson_cnn_amd import ops
    _, dev = _inputs(H, W)
    pred, target, rho, rhs, dx = dev
    old = ops.varcoef_error_stats(pred, rho, target, rhs, dx).cpu().numpy()
    assert np.array_equal(bits(_raw(0, H, W, *dev)), bits(old)) and np.all(old[:, 5:] > 0)
    assert np.array_equal(bits(_call(0, *dev)), bits(old)) and np.array_equal(bits(_call((False,) * 4, *dev)), bits(old))


@pytest.mark.parametrize('mask', [5, 15])
def test_equal_inputs_give_equal_bits_and_null_fields_zero_their_columns(mask):
    from poisson_cnn_amd import ops
    H, W = 70, 133
    _, dev = _inputs(H, W)
    pred, target, rho, rhs, dx = dev
    got = _call(mask, *dev)
    assert np.array_equal(bits(_call(mask, *dev)), bits(got))
    assert np.array_equal(bits(_raw(mask, H, W, *dev)), bits(got))
    flags = tuple(bool(mask >> k & 1) for k in range(4))                                        # the four-flag spelling of the mask
    assert np.array_equal(bits(_call(flags, *dev)), bits(got))
    no_t = _call(mask, pred, None, rho, rhs, dx)
    assert np.all(no_t[:, :5] == 0.0) and np.array_equal(bits(no_t[:, 5:]), bits(got[:, 5:]))
    for r in (rho, None):                                                                       # without rhs, rho and dx are not read
        no_f = ops.varcoef_error_stats(pred, r, target, neumann_mask=mask).cpu().numpy()
        assert np.all(no_f[:, 5:] == 0.0) and np.array_equal(bits(no_f[:, :5]), bits(got[:, :5]))
    assert np.array_equal(bits(_raw(mask, H, W, pred, target, None, None, None)[:, :5]), bits(got[:, :5]))
    assert np.all(ops.varcoef_error_stats(pred, None, neumann_mask=mask).cpu().numpy() == 0.0)


@pytest.mark.parametrize('H,W', [(3, 3), (70, 133)])
def test_samples_do_not_see_each_other(H, W):
    """The other sample filled with 1e30 in all four fields: a neighbour or a mirrored index taken from it would show."""
    _, dev = _inputs(H, W)
    got = _call(15, *dev)
    for keep in (0, 1):
        big = [t.clone() for t in dev[:4]]
        for t in big:
            t[1 - keep] = 1e30
        assert np.array_equal(bits(_call(15, *big, dev[4])[keep]), bits(got[keep]))


def test_the_library_refuses_a_bad_mask_and_a_grid_without_unknowns():
    _, dev = _inputs(9, 11)
    for bad in (16, -1):
        with pytest.raises(RuntimeError, match='pcnn_varcoef_bc_error_stats: neumann_mask'):
            _raw(bad, 9, 11, *dev)
    two = [t[:, :2, :5].contiguous() for t in dev[:4]]
    with pytest.raises(RuntimeError, match='H, W >= 3'):                     # the mirrored index of a 2-point axis would be the node itself
        _raw(15, 2, 5, *two, dev[4])
    with pytest.raises(RuntimeError, match='rhs needs rho'):
        _raw(5, 9, 11, dev[0], dev[1], None, dev[3], dev[4])
    assert np.all(_raw(5, 9, 11, *dev)[:, 5:] > 0)                           # the handle is usable afterwards


# ----------------------------------------------------------------------------- the model with residual_metrics=True
TYPES = [None] + VB.TYPES                       # all Dirichlet (the keyword absent), left + top Neumann (mask 9), all four Neumann (mask 15)
IDS = ['dirichlet'] + VB.IDS


def _cfg(bt, **kw):
    return VM.model_cfg(2, density_input=True, **({} if bt is None else {'boundary_types': bt}), **kw)


def _compiled(bt, **kw):
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    model = VM.build(_cfg(bt, **kw))[0]
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=VM.N, boundary_types=bt, **VM.loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3))
    return model


def _twin_of(model, bt):
    """the float32-order twin on the model's own fp32 output: (N, 8)"""
    stack, dx, target = VM.batch()
    y = model([stack, dx]).cpu().numpy()
    assert y.dtype == np.float32
    return ST.error_stats(y[:, 0], stack[:, 1], target[:, 0], stack[:, 0], dx[:, 0], 0 if bt is None else E.mask_of(bt), float32_terms=True)


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_evaluate_and_predict_report_the_flux_form_residual(bt):
    stack, dx, target = VM.batch()
    assert np.all((stack[:, 0, 1:-1, 1:-1] != 0).any(axis=(1, 2)))           # nonzero right-hand sides: no sample may be skipped
    model = _compiled(bt, residual_metrics=True)
    tw = _twin_of(model, bt)
    tol = sum_tol(VM.H, VM.W)
    res = model.evaluate([stack, dx], target, batch_size=VM.N, return_dict=True, per_sample=True)
    s = res['stats']
    assert res['skipped_rel_residual'] == 0 and res['samples'] == VM.N
    assert s.shape == (VM.N, 8) and np.array_equal(s[:, 6], tw[:, 6])
    assert np.all(np.abs(s[:, SUMS] - tw[:, SUMS]) <= tol * tw[:, SUMS])
    # sqrt(a (1 + d1) / (b (1 + d2))) = sqrt(a / b) (1 + (d1 - d2) / 2 + ...), |d| <= tol: the same bound holds for the ratio's root and for the mean
    rel = float(np.mean(np.sqrt(tw[:, 5] / tw[:, 7])))
    print('%s: rel_residual %.9g vs twin %.9g (difference / tolerance %.3g)' % (bt, res['rel_residual'], rel, abs(res['rel_residual'] - rel) / (tol * rel)))
    assert abs(res['rel_residual'] - rel) <= tol * rel
    pred, stats3 = model.predict([stack, dx], batch_size=VM.N, return_stats=True)
    assert stats3.shape == (VM.N, 3) and np.array_equal(stats3, s[:, 5:])
    assert np.array_equal(pred, model([stack, dx]).cpu().numpy())


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_fit_logs_a_finite_val_rel_residual_a_callback_can_monitor(bt):
    from poisson_cnn_amd.train import EarlyStopping
    stack, dx, target = VM.batch()

    class Seq:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return (stack, dx), target
    model = _compiled(bt, residual_metrics=True)
    stop = EarlyStopping(monitor='val_rel_residual', patience=5)
    hist = model.fit(Seq(), epochs=2, verbose=0, validation_data=([stack, dx], target), validation_batch_size=VM.N, callbacks=[stop])
    v = hist['val_rel_residual']
    assert len(v) == 2 and all(np.isfinite(x) and x > 0 for x in v) and v[0] != v[1]
    assert stop.best in v                                                    # the callback found its monitor


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_solve_returns_the_max_residual_with_neumann_edges_too(bt):
    stack, dx, _ = VM.batch()
    model = VM.build(_cfg(bt, residual_metrics=True))[0]
    plain = VM.build(_cfg(bt))[0]
    info, ref = model.solve([stack, dx], return_info=True)[1], plain.solve([stack, dx], return_info=True)[1]
    tw = _twin_of(model, bt)
    got = info['prediction_max_residual']
    assert isinstance(got, np.ndarray) and got.shape == (VM.N,) and np.array_equal(got, tw[:, 6])
    # the relative residual keeps its source and its bits
    assert np.array_equal(info['prediction_relative_residual'], ref['prediction_relative_residual']) and np.all(np.isfinite(got))
    assert np.array_equal(info['iterations'], ref['iterations'])


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_defaults_are_unchanged(bt):
    stack, dx, target = VM.batch()
    model = _compiled(bt)
    assert model.residual_metrics is False
    res = model.evaluate([stack, dx], target, batch_size=VM.N, return_dict=True, per_sample=True)
    assert (res['stats'][:, 5:] == 0).all() and (res['stats'][:, :5] > 0).all()
    assert np.isnan(res['rel_residual']) and res['skipped_rel_residual'] == VM.N
    info = model.solve([stack, dx], return_info=True)[1]
    assert (info['prediction_max_residual'] is None) == (bt is not None)


def test_a_checkpoint_holds_no_trace_of_the_keyword(tmp_path):
    stack, dx, _ = VM.batch()
    bt = VB.TYPES[0]
    a, b = VM.build(_cfg(bt, residual_metrics=True))[0], VM.build(_cfg(bt), seed=99)[0]
    a.save_weights(str(tmp_path / 'w'))
    b.load_weights(str(tmp_path / 'w'))
    assert a.store.trainable_names() == b.store.trainable_names() and torch.equal(a.store.flat_w, b.store.flat_w)
    assert torch.equal(a([stack, dx]), b([stack, dx]))
