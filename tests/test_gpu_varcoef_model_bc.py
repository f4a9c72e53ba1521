"""Homogeneous_Poisson_NN_Legacy(density_input=True, boundary_types=...), losses.variable_density_loss_wrapper(boundary_types=...), model.solve and
`train --dataset_type variable_density` with per-edge Neumann boundaries: the tiny model and the 2 x 24 x 28 batch of
tests/test_gpu_varcoef_model.py with three smoother sweeps, left + top Neumann (mask 9) and all four edges Neumann (mask 15).

The fp64 restatement is varcoef_train_twin.model_forward without its smoother (its zero ring leaves the interior as it is), then the per-edge ring of
tests/bc_edges_twin.py and the sweeps of tests/varcoef_train_bc_twin.py as dense matrices, which torch differentiates.  Bounds: the tiny-config ones
of tests/test_gpu_varcoef_model.py (forward 1e-5, flat gradient 2e-4, loss 2e-5) and of tests/test_gpu_varcoef_solve.py (solution 2e-7)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import np_ops, torch_twin
from tests import bc_edges_twin as E, test_gpu_varcoef_model as VM, varcoef_bc_twin as B, varcoef_train_bc_twin as BT, varcoef_train_twin as T

pytestmark = pytest.mark.gpu
N, H, W = VM.N, VM.H, VM.W
TYPES = [{'left': 'neumann', 'top': 'neumann'}, {'left': 'neumann', 'right': 'neumann', 'bottom': 'neumann', 'top': 'neumann'}]
IDS = ['left+top', 'all-four']
SWEEPS = 3


def cfg_of(bt, iterations=SWEEPS):
    return VM.model_cfg(iterations, density_input=True, boundary_types=bt)


@functools.lru_cache(maxsize=None)
def _dense(mask):
    """Per sample of VM.batch(): (J, scale, L, w) as float64 torch tensors - the one-sweep matrix, its rhs scale, the (unknowns x H W) operator, w."""
    stack, dx, _ = VM.batch()
    out = []
    for n in range(N):
        J, scale = BT.sweep_matrix(stack[n, 1], float(dx[n, 0]), mask)
        L, _ = BT.operator_matrix(stack[n, 1], float(dx[n, 0]), mask)
        out.append(tuple(torch.tensor(a) for a in (J.toarray(), scale, L.toarray(), B.weights(H, W, mask).ravel())))
    return out


def forward_twin(ops_, cfg, p, stack, dx):
    """The model in fp64: numpy with oracle.np_ops, differentiable torch with oracle.torch_twin."""
    mask = E.mask_of(cfg['boundary_types'])
    base = {k: v for k, v in cfg.items() if k != 'boundary_types'}
    x = E.ring(T.model_forward(ops_, dict(base, postsmoother_iterations=0), p, stack, dx), mask)
    as_t = isinstance(x, torch.Tensor)
    rows = []
    for n, (J, scale, _, _) in enumerate(_dense(mask)):
        v = (x[n, 0] if as_t else torch.tensor(x[n, 0])).reshape(-1)
        c = scale * torch.tensor(np.asarray(stack[n, 0], dtype=np.float64)).reshape(-1)
        for _ in range(cfg['postsmoother_iterations']):
            v = J @ v - c
        rows.append(v.reshape(1, H, W))
    out = torch.stack(rows)
    return out if as_t else out.numpy()


def loss_twin(lossp, gbs, y_true, y_pred, stack, dx, mask):
    """variable_density_loss_wrapper(boundary_types=...) in fp64 torch: the oracle's supervised terms + weight / (N sum w) * sum of w (L pred - f)^2."""
    loss = T.density_loss(dict(lossp, physics_informed_loss_weight=0.0), gbs, y_true, y_pred, stack, dx)
    si, sj = BT.unknown_slices(H, W, mask)
    for n, (_, _, L, w) in enumerate(_dense(mask)):
        r = L @ y_pred[n, 0].reshape(-1) - torch.tensor(np.asarray(stack[n, 0], dtype=np.float64)[si, sj]).reshape(-1)
        loss = loss + float(lossp['physics_informed_loss_weight']) * (w * r * r).sum() / (N * float(w.sum()))
    return loss


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_forward_and_gradient_against_the_fp64_twin(bt):
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import SGD
    stack, dx, target = VM.batch()
    cfg, mask = cfg_of(bt), E.mask_of(bt)
    model, p = VM.build(cfg)
    assert model.neumann_mask == mask and model.postsmoother.neumann_mask == mask
    ref = forward_twin(np_ops, cfg, p, stack, dx)
    y = model([stack, dx]).cpu().numpy()
    err = VM.rel(y, ref)
    print('forward vs fp64 twin, mask %d: rel-L2 %.3g' % (mask, err))
    assert y.shape == ref.shape and err <= VM.TOL_FWD
    # the smoother moved the Neumann edges off the ring's mirror values, and left the Dirichlet edges at zero
    ring_only = VM.build(cfg_of(bt, 0))[0]([stack, dx]).cpu().numpy()
    assert np.abs(y[:, 0, 0, 1:-1] - ring_only[:, 0, 0, 1:-1]).max() > 0
    if mask != 15:
        assert not y[:, 0, -1, :].any() and not y[:, 0, :, 0].any()
    # the residual is of order 1 / dx^2: the weight is set from the twin so that the physics-informed term equals the supervised ones
    unit = VM.loss_params(1.0)
    supervised = float(loss_twin(dict(unit, physics_informed_loss_weight=0.0), 4, target, torch.tensor(ref), stack, dx, mask))
    lossp = VM.loss_params(float(np.float32(supervised / (float(loss_twin(unit, 4, target, torch.tensor(ref), stack, dx, mask)) - supervised))))
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=not k.endswith(('moving_mean', 'moving_variance'))) for k, v in p.items()}
    pred = forward_twin(torch_twin, cfg, pt, torch.tensor(stack), torch.tensor(dx))
    loss = loss_twin(lossp, 4, target, pred, stack, dx, mask)
    loss.backward()
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=4, boundary_types=bt, **lossp), optimizer=SGD(learning_rate=0.0))
    logs = model.train_step(((stack, dx), target))
    names = model.store.trainable_names()
    flat = np.concatenate([model.store.g[n].cpu().numpy().ravel() for n in names])
    flat_ref = np.concatenate([pt[n].grad.numpy().ravel() for n in names])
    gerr = VM.rel(flat, flat_ref)
    print('mask %d: loss %.6g vs %.6g, flat gradient rel-L2 %.3g' % (mask, float(logs['loss']), float(loss.detach()), gerr))
    assert abs(float(logs['loss']) - float(loss.detach())) <= 2e-5 * abs(float(loss.detach()))
    assert gerr <= VM.TOL_GRAD
    assert abs(float(loss.detach()) - 2.0 * supervised) <= 1e-3 * supervised                 # both halves of the loss are in this gradient


def test_all_dirichlet_boundary_types_give_the_bits_of_the_model_without_the_keyword():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import SGD
    stack, dx, target = VM.batch()
    grads = []
    for kw in ({}, {'boundary_types': dict.fromkeys(B.EDGES, 'dirichlet')}, {'boundary_types': {}}):
        model = VM.build(VM.model_cfg(SWEEPS, density_input=True, **kw))[0]
        assert model.neumann_mask == 0
        y = model([stack, dx])
        model.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **VM.loss_params(1e-9), **kw), optimizer=SGD(learning_rate=0.0))
        logs = model.train_step(((stack, dx), target))
        grads.append((y, model.store.flat_g.clone(), float(logs['loss'])))
    for y, g, loss in grads[1:]:
        assert torch.equal(y, grads[0][0]) and torch.equal(g, grads[0][1]) and loss == grads[0][2]


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_adam_lowers_the_loss_on_a_generator_batch(bt):
    from poisson_cnn_amd import dataset as D
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    gen = D.variable_density_dataset_generator(batch_size=2, output_shape=(H, W), seed=7, boundary_types=bt)
    (stack, dx), soln = gen[0]
    model = VM.build(cfg_of(bt, 2))[0]
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=2, boundary_types=bt, **VM.loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3))
    losses = [float(model.train_step(((stack, dx), soln))['loss']) for _ in range(10)]
    print('ten Adam steps, %r: loss %.6g -> %.6g' % (sorted(bt), losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


@functools.lru_cache(maxsize=None)
def _solution(mask):
    stack, dx, _ = VM.batch()
    zero = {'left': np.zeros((N, W)), 'right': np.zeros((N, W)), 'bottom': np.zeros((N, H)), 'top': np.zeros((N, H))}
    return zero, B.solve_batch(stack[:, 1], stack[:, 0], zero, dx[:, 0], mask)


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_solve_starts_the_neumann_solve_from_the_prediction(bt):
    from poisson_cnn_amd import dataset as D
    stack, dx, _ = VM.batch()
    mask = E.mask_of(bt)
    zero, ref = _solution(mask)
    m = VM.build(cfg_of(bt, 2))[0]
    soln, info = m.solve([stack, dx], return_info=True)
    pred = m([stack, dx])
    direct = D.variable_density_poisson_solve(stack[:, 1], stack[:, 0], zero, dx[:, 0], boundary_types=bt, initial_guesses=pred, check_start=True)
    assert torch.equal(soln, direct)                                                         # the same start, the same solve: bit for bit
    err = VM.rel(soln.cpu().numpy()[:, 0], ref)
    print('solve, mask %d: rel-L2 vs the direct fp64 solve %.3g after %r iterations' % (mask, err, info['iterations'].tolist()))
    assert info['converged'].all() and err <= 2e-7
    # the residual the solve starts from, against the twin on the model's own fp32 output
    p64 = pred.cpu().numpy().astype(np.float64)[:, 0]
    w = B.weights(H, W, mask)
    si, sj = BT.unknown_slices(H, W, mask)
    tw = np.array([np.sqrt(BT.loss(p64[n], stack[n, 1], stack[n, 0], float(dx[n, 0]), mask) / float((w * stack[n, 0][si, sj] ** 2).sum())) for n in range(N)])
    got = info['prediction_relative_residual']
    print('prediction_relative_residual %r vs twin %r' % (got.tolist(), tw.tolist()))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - tw) <= 2e-5 * tw)
    assert info['prediction_max_residual'] is None
    assert 'cold_iterations' not in info
    cold = m.solve([stack, dx], return_info=True, compare_cold=True, check_every=4)[1]['cold_iterations']
    assert cold.shape == (N,) and np.all(cold > 0) and np.all(cold % 4 == 0)


@pytest.mark.parametrize('bt', TYPES, ids=IDS)
def test_a_start_at_the_solution_needs_no_iteration(bt):
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    stack, dx, _ = VM.batch()
    ref = _solution(E.mask_of(bt))[1]

    class Exact(Homogeneous_Poisson_NN_Legacy):
        def call(self, inp, training=False):
            return torch.tensor(ref[:, None], dtype=torch.float64, device=self.device)

    soln, info = Exact(**cfg_of(bt, 2)).solve([stack, dx], return_info=True, check_every=4)
    assert (info['iterations'] == 0).all() and info['converged'].all()
    assert VM.rel(soln.cpu().numpy()[:, 0], ref) <= 2e-7


def test_checkpoints_round_trip_keeps_the_keyword(tmp_path):
    stack, dx, _ = VM.batch()
    cfg = cfg_of(TYPES[0], 2)
    a = VM.build(cfg)[0]
    a.save_weights(str(tmp_path / 'w'))
    b = VM.build(cfg, seed=99)[0]
    b.load_weights(str(tmp_path / 'w'))
    assert b.neumann_mask == a.neumann_mask == 9 and b.boundary_types == a.boundary_types
    assert torch.equal(a([stack, dx]), b([stack, dx]))
    plain = VM.build(VM.model_cfg(2, density_input=True), seed=99)[0]                      # the same weights without the keyword: another model
    plain.load_weights(str(tmp_path / 'w'))
    assert not torch.equal(plain([stack, dx]), a([stack, dx]))
    (dummy, ddx), dtarget = a._dummy_batch((N, H, W))                                        # presize's batch is the two-channel one
    assert tuple(dummy.shape) == (N, 2, H, W)


def test_train_main_runs_two_steps_with_neumann_edges_in_both_sections(tmp_path, monkeypatch):
    from poisson_cnn_amd import configs, dataset as D, losses, models as M, train
    bt = TYPES[0]
    cfg = configs.hpnn_tiny()
    cfg['model'].update(density_input=True, postsmoother_iterations=2, boundary_types=bt)
    cfg['dataset'] = {'batch_size': 2, 'batches_per_epoch': 2, 'output_shape': [H, W], 'boundary_types': dict(bt, right='dirichlet')}
    cfg['training']['n_epochs'] = 1
    cfg['training']['loss_parameters'] = VM.loss_params(1e-9)
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    seen = {}
    orig_fit = M.Homogeneous_Poisson_NN_Legacy.fit

    def fit(self, dataset, *a, **kw):
        seen['model'], seen['dataset'] = self, dataset
        seen['history'] = orig_fit(self, dataset, *a, **kw)
        return seen['history']
    monkeypatch.setattr(M.Homogeneous_Poisson_NN_Legacy, 'fit', fit)
    train.main([str(path), '--dataset_type', 'variable_density', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    model = seen['model']
    assert model.neumann_mask == 9 and isinstance(model.loss_fn, losses.variable_density_loss_wrapper) and model.loss_fn.neumann_mask == 9
    assert isinstance(seen['dataset'], D.variable_density_dataset_generator) and seen['dataset'].neumann_flags == (True, False, False, True)
    assert model.optimizer.iterations == 2 and all(np.isfinite(v) for v in seen['history']['loss'])
    assert any(f.startswith('chkpt') for f in os.listdir(tmp_path))
    # a dataset section without the key is filled in from the model section
    del cfg['dataset']['boundary_types']
    path.write_text(json.dumps(cfg))
    train.main([str(path), '--dataset_type', 'variable_density', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    assert seen['dataset'].neumann_flags == (True, False, False, True)
