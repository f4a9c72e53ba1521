"""tests/varcoef_error_stats_bc_twin.py against the twins it is built on, and the host-side refusals of the residual metrics.
No GPU: the kernel itself is tests/test_gpu_varcoef_error_stats_bc.py's."""
import json

import numpy as np
import pytest

from tests import error_stats_twin as TW, varcoef_bc_twin as B, varcoef_error_stats_bc_twin as ST, varcoef_train_bc_twin as BT

SHAPES = [(3, 3), (3, 4), (9, 11)]
MASKS = list(range(16))
N = 2


def _fields(seed, H, W):
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                          # fp32-representable values: both dtypes of the twin see the same inputs
    return (f32(rng.uniform(-1, 1, (N, H, W))), f32(rng.uniform(-1, 1, (N, H, W))), f32(rng.uniform(1.0, 10.0, (N, H, W))),
            f32(rng.standard_normal((N, H, W)) * 50), f32(rng.uniform(5e-3, 5e-2, (N,))))


@pytest.mark.parametrize('H,W', SHAPES)
def test_mask_0_is_the_all_dirichlet_twin(H, W):
    """All eight columns.  float32 terms: the same operations in the same order, so the same numbers; float64: the assembled system against the
    explicit formula, equal up to the order of the fp64 operations (1e-11 of a column)."""
    pred, target, rho, rhs, dx = _fields(41, H, W)
    got32 = ST.error_stats(pred, rho, target, rhs, dx, 0, float32_terms=True)
    assert np.array_equal(got32, TW.error_stats(pred, target, rhs, dx, rho, float32_terms=True))
    got, ref = ST.error_stats(pred, rho, target, rhs, dx, 0), TW.error_stats(pred, target, rhs, dx, rho)
    assert np.all(ref > 0) and np.all(np.abs(got - ref) <= 1e-11 * ref)
    no_rhs = ST.error_stats(pred, None, target)
    assert np.array_equal(no_rhs[:, :5], ref[:, :5]) and not no_rhs[:, 5:].any()


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_weighted_sums_are_the_training_loss(H, W, mask):
    """Column 5 is varcoef_train_bc_twin.loss - the sum of w r^2 the training loss divides by its normaliser weight_sum - and column 7 the same
    weighted sum of f^2; the float32-order residual, stated with mirrored indices, is that loss's r (1e-11 in float64, fp32 rounding in float32)."""
    pred, target, rho, rhs, dx = _fields(42 + mask, H, W)
    loss = BT.loss_batch(pred, rho, rhs, dx, mask)
    w = B.weights(H, W, mask)
    si, sj = BT.unknown_slices(H, W, mask)
    ff = np.array([(w * rhs[n].astype(np.float64)[si, sj] ** 2).sum() for n in range(N)])
    assert w.shape == (si.stop - si.start, sj.stop - sj.start) and w.sum() == BT.weight_sum(H, W, mask)
    got = ST.error_stats(pred, rho, target, rhs, dx, mask)
    assert np.all(np.abs(got[:, 5] - loss) <= 1e-12 * loss) and np.all(np.abs(got[:, 7] - ff) <= 1e-12 * ff)
    for n in range(N):
        ref = BT.residual(pred[n], rho[n], rhs[n], float(dx[n]), mask)
        r64 = ST.ordered_residual(pred[n], rho[n], rhs[n], dx[n], mask)
        assert r64.shape == ref.shape and np.abs(r64 - ref).max() <= 1e-11 * np.abs(ref).max()
        assert got[n, 6] == np.abs(ref).max()
    got32 = ST.error_stats(pred, rho, target, rhs, dx, mask, float32_terms=True)
    assert np.all(np.abs(got32[:, 5] - loss) <= 1e-4 * loss) and np.all(np.abs(got32[:, 7] - ff) <= 1e-12 * ff)
    assert np.array_equal(got32[:, :5], TW.error_stats(pred, target, float32_terms=True)[:, :5])


def test_refusals_on_the_host():
    from poisson_cnn_amd import configs, ops
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    cfg = configs.hpnn_tiny()['model']
    with pytest.raises(ValueError, match='residual_metrics'):                # the constant-coefficient model reports its 3 x 3 residual already
        Homogeneous_Poisson_NN_Legacy(**dict(cfg, residual_metrics=True))
    for bad in (16, -1, (True, False, True)):
        with pytest.raises(ValueError, match='neumann_mask'):
            ops.varcoef_error_stats(None, None, neumann_mask=bad)           # refused before any tensor is looked at


def test_the_keyword_survives_a_config_round_trip(tmp_path):
    from poisson_cnn_amd import configs
    cfg = configs.hpnn_tiny()
    cfg['model'].update(density_input=True, boundary_types={'left': 'neumann'}, residual_metrics=True)
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    back = configs.load_config(str(path))
    assert back['model']['residual_metrics'] is True and back['model'] == cfg['model']
