"""The fp64 twin of the variable-density training operators with per-edge Neumann boundaries (tests/varcoef_train_bc_twin.py)
against what the project already trusts: the all-Dirichlet twin tests/varcoef_train_twin.py, the solver's twin tests/varcoef_bc_twin.py (its assembled
system, its direct solve, its constant-coefficient operator) and a finite difference of the loss; then the host-side refusals of the new keyword.
CPU only.  All 16 masks at 3 x 3 (every node an unknown at mask 15), 3 x 4 and 9 x 11."""
import json

import numpy as np
import pytest

from tests import varcoef_bc_twin as B
from tests import varcoef_train_bc_twin as BT
from tests import varcoef_train_twin as T

SHAPES = [(3, 3), (3, 4), (9, 11)]
MASKS = list(range(16))


def _fields(seed, H, W):
    rng = np.random.default_rng(seed)
    u, f, g = (rng.standard_normal((H, W)) for _ in range(3))
    return u, rng.uniform(1.0, 10.0, (H, W)), f, g, float(rng.uniform(5e-3, 5e-2))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize('H,W', SHAPES)
def test_mask_0_is_the_all_dirichlet_twin(H, W):
    """Loss, gradient, sweeps and adjoint: the same numbers up to the order of the fp64 sums (1e-12; nothing else differs)."""
    u, rho, f, g, dx = _fields(11, H, W)
    t = lambda a: T.t64(a[None])
    d = T.t64([dx])
    assert abs(BT.loss(u, rho, f, dx, 0) - float(T.residual_loss(t(u), t(rho), t(f), d)[0])) <= 1e-12 * BT.loss(u, rho, f, dx, 0)
    assert _rel(BT.loss_grad(u, rho, f, dx, 0), T.residual_loss_grad(t(u), t(rho), t(f), d, T.t64([1.0]))[0].numpy()) <= 1e-12
    for n in (1, 3):
        assert _rel(BT.sweep(u, rho, f, dx, 0, n), T.sweep(t(u), t(rho), t(f), d, n)[0].numpy()) <= 1e-12
        assert _rel(BT.sweep_adjoint(g, rho, dx, 0, n), T.sweep_adjoint(t(g), t(rho), d, n)[0].numpy()) <= 1e-12


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_residual_of_the_assembled_system_is_the_explicit_operator(H, W, mask):
    """b - A x of varcoef_bc_twin.assemble with the field's own Dirichlet values is L pred - f with the (unknowns x H W) matrix assembled here."""
    u, rho, f, _, dx = _fields(12 + mask, H, W)
    L, _ = BT.operator_matrix(rho, dx, mask)
    si, sj = BT.unknown_slices(H, W, mask)
    assert _rel(BT.residual(u, rho, f, dx, mask).ravel(), L @ u.ravel() - f[si, sj].ravel()) <= 1e-12


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_gradient_is_the_central_difference_of_the_loss(H, W, mask):
    """The loss is quadratic in pred, so the central difference is exact for every step; step 1 - a power of two on fields of unit scale, so pred +- step
    is formed without rounding and the difference of the two losses loses about 1e-14 of the gradient's size."""
    u, rho, f, _, dx = _fields(13 + mask, H, W)
    grad = BT.loss_grad(u, rho, f, dx, mask)
    fd = np.zeros_like(grad)
    for i in range(H):
        for j in range(W):
            e = np.zeros((H, W))
            e[i, j] = 1.0
            fd[i, j] = (BT.loss(u + e, rho, f, dx, mask) - BT.loss(u - e, rho, f, dx, mask)) / 2.0
    assert np.abs(grad).max() > 0 and _rel(grad, fd) <= 1e-6


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_adjoint_identity(H, W, mask):
    u, rho, f, g, dx = _fields(14 + mask, H, W)
    for n in (1, 4):
        lin = BT.sweep(u, rho, f, dx, mask, n) - BT.sweep(np.zeros_like(u), rho, f, dx, mask, n)
        lhs, rhs = float((BT.sweep_adjoint(g, rho, dx, mask, n) * u).sum()), float((g * lin).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(rhs), np.linalg.norm(g) * np.linalg.norm(lin) * 1e-3)
    # a Dirichlet node keeps its own g, an unknown does not: with g the indicator of one node, one sweep
    si, sj = BT.unknown_slices(H, W, mask)
    unknown = np.zeros((H, W), dtype=bool)
    unknown[si, sj] = True
    for (i, j) in ((0, 0), (1, 1), (0, W // 2), (H - 1, W - 1)):
        e = np.zeros((H, W))
        e[i, j] = 1.0
        assert BT.sweep_adjoint(e, rho, dx, mask)[i, j] == (0.0 if unknown[i, j] else 1.0)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_direct_solution_is_a_fixed_point_of_the_sweep(H, W, mask):
    """varcoef_bc_twin.solve with random Dirichlet data and g = 0; mask 15: of the projected right-hand side, f + the shift of the projection."""
    rng = np.random.default_rng(15 + mask)
    _, rho, f, _, dx = _fields(16 + mask, H, W)
    flags = B.flags(mask)
    bnd = {e: (np.zeros(n) if fl else rng.standard_normal(n)) for e, fl, n in zip(B.EDGES, flags, (W, W, H, H))}
    u = B.solve(rho, f, bnd, dx, mask)
    if mask == 15:
        _, b = B.assemble(rho, dx, mask, bnd, f)
        f = -B.project(b, B.weights(H, W, mask))[0].reshape(H, W)
    assert _rel(BT.sweep(u, rho, f, dx, mask, 1), u) <= 1e-10


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_constant_density_is_the_constant_coefficient_neumann_operator(H, W, mask):
    c, dx = 3.5, 0.02
    L, diag = BT.operator_matrix(np.full((H, W), c), dx, mask)
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    node = (np.arange(i0, i1 + 1)[:, None] * W + np.arange(j0, j1 + 1)[None, :]).ravel()
    M = B.constant_operator(H, W, mask)
    assert _rel(-(L.toarray()[:, node]) * dx * dx * c, M) <= 1e-12
    assert _rel(diag * dx * dx * c, np.diag(M)) <= 1e-12
    assert abs(BT.weight_sum(H, W, mask) - (H - 2 + 0.5 * (mask & 1) + 0.5 * (mask >> 1 & 1)) * (W - 2 + 0.5 * (mask >> 2 & 1) + 0.5 * (mask >> 3 & 1))) == 0.0


# ----------------------------------------------------------------------------- host-side refusals
def _loss_params():
    from poisson_cnn_amd import configs
    lossp = dict(configs.hpnn_tiny()['training']['loss_parameters'])
    lossp.update(physics_informed_loss_weight=1e-9, physics_informed_loss_config={'stencil_sizes': [3, 3], 'orders': 2, 'normalize': False})
    return lossp


def test_loss_keyword():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    for mask in MASKS:
        loss = variable_density_loss_wrapper(boundary_types=B.types(mask), **_loss_params())
        assert loss.neumann_mask == mask
        for H, W in SHAPES:
            assert float(loss.weight_sum(H, W)) == BT.weight_sum(H, W, mask)
    assert variable_density_loss_wrapper(**_loss_params()).neumann_mask == 0
    for bad in ({'front': 'neumann'}, {'left': 'robin'}, 'neumann', ['left']):
        with pytest.raises(ValueError, match='boundary_types'):
            variable_density_loss_wrapper(boundary_types=bad, **_loss_params())


def test_layer_keyword():
    from poisson_cnn_amd.layers import VariableDensityJacobiLayer
    assert VariableDensityJacobiLayer(3).neumann_mask == 0
    assert VariableDensityJacobiLayer(3, boundary_types={'left': 'neumann', 'top': 'Neumann', 'right': 'dirichlet'}).neumann_mask == 9
    for bad in ({'front': 'neumann'}, {'left': 'robin'}, 'neumann'):
        with pytest.raises(ValueError, match='boundary_types'):
            VariableDensityJacobiLayer(3, boundary_types=bad)


def test_model_keyword_refusals():
    from poisson_cnn_amd import configs
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    cfg = configs.hpnn_tiny()['model']
    with pytest.raises(ValueError, match='bc_type'):                       # the constant-coefficient model's keyword is bc_type
        Homogeneous_Poisson_NN_Legacy(**dict(cfg, boundary_types={'left': 'neumann'}))
    for bad in ({'front': 'neumann'}, {'left': 'robin'}, 'neumann'):
        with pytest.raises(ValueError, match='boundary_types'):
            Homogeneous_Poisson_NN_Legacy(**dict(cfg, density_input=True, boundary_types=bad))
    with pytest.raises(NotImplementedError, match='density_input'):        # bc_type stays refused, with or without the new keyword
        Homogeneous_Poisson_NN_Legacy(**dict(cfg, density_input=True, bc_type='neumann', boundary_types={'left': 'neumann'}))


def _train(tmp_path, model_bt, dataset_bt):
    from poisson_cnn_amd import configs, train
    cfg = configs.hpnn_tiny()
    cfg['model']['density_input'] = True
    if model_bt is not None:
        cfg['model']['boundary_types'] = model_bt
    cfg['dataset'] = {'batch_size': 2}
    if dataset_bt is not None:
        cfg['dataset']['boundary_types'] = dataset_bt
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    train.main([str(path), '--dataset_type', 'variable_density', '--model', 'hpnn'])


def test_train_wants_the_two_sections_to_name_the_same_edges(tmp_path):
    with pytest.raises(ValueError, match='model does not') as info:
        _train(tmp_path, None, {'left': 'neumann'})
    assert 'boundary_types' in str(info.value).split('drop boundary_types')[1]         # the remedy names the model's keyword
    for model_bt, dataset_bt in (({'left': 'neumann'}, {'right': 'neumann'}), ({'left': 'neumann'}, {'left': 'neumann', 'top': 'neumann'}),
                                 ({'left': 'neumann'}, {'left': 'dirichlet'})):
        with pytest.raises(ValueError, match='model section') as info:
            _train(tmp_path, model_bt, dataset_bt)
        assert repr(model_bt) in str(info.value) and repr(dataset_bt) in str(info.value)
    with pytest.raises(ValueError, match='boundary_types'):
        _train(tmp_path, 'neumann', None)
