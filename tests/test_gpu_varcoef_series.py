"""pcnn_varcoef_series_pair (one launch: a series solution synthesised in fp64 and the discrete flux-form right-hand side differenced from it),
ops.varcoef_series_pair, dataset.reverse_variable_density_dataset_generator and `train --dataset_type variable_density_analytical` (DESIGN.md
section 23) against the fp64 twin of tests/varcoef_series_twin.py.

Shapes 33 x 47, 45 x 70 and 97 x 65: none a multiple of the 16 x 64 tile, one narrower than a tile, one more than a tile both ways.  Batch 3 with
three spacings, rho from pcnn_varcoef_density at ratio 1000, 5 x 8 and 16 x 16 modes, masks 0, 1, 6, 15.
Bounds: 2e-6 rel-L2 against the twin (the per-op bound; the route that differences a float32 u is off by 2.3e-5 at 97 x 65,
tests/test_varcoef_series_reference.py); the consistency floor eps32 * 8 * max(beta) * max|u| / dx^2 worked out per sample; the round trip through
variable_density_poisson_solve within 4 x the twin's own round-trip figure for the very rho of the test."""
import functools
import json
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B, varcoef_series_twin as S, varcoef_train_bc_twin as BT

pytestmark = pytest.mark.gpu
PER_OP = 2e-6
MASKS = (0, 1, 6, 15)
N = 3
CASES = [(s, m, k) for s in range(len(S.SHAPES)) for m in range(len(S.MODES)) for k in MASKS]
case_id = lambda c: '%dx%d-%dx%d-mask%d' % (S.SHAPES[c[0]] + S.MODES[c[1]] + (c[2],))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), device='cuda', dtype=dtype).contiguous()


@functools.lru_cache(maxsize=None)
def density(s):
    """(device rho from pcnn_varcoef_density at ratio 1000, its host copy) for shape s."""
    from poisson_cnn_amd.dataset import _kernels as K
    rho = K.varcoef_density(dev(S.smooth_unit_field(N, *S.SHAPES[s])), 1.0, S.RATIO)
    return rho, rho.cpu().numpy()


@functools.lru_cache(maxsize=None)
def launch(s, m, mask):
    """(soln, rhs) device tensors of one launch."""
    from poisson_cnn_amd import ops
    return ops.varcoef_series_pair(dev(S.coefficients(N, *S.MODES[m])), density(s)[0], dev(S.DX), mask)


@functools.lru_cache(maxsize=None)
def reference(s, m, mask):
    return S.twin(S.coefficients(N, *S.MODES[m]), density(s)[1], np.array(S.DX), mask)


@functools.lru_cache(maxsize=None)
def round_trip_figure(s, m, mask):
    return S.round_trip(S.coefficients(N, *S.MODES[m]), density(s)[1], np.array(S.DX), mask)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_twin_parity_and_exact_zeros(case):
    s, m, mask = case
    H, W = S.SHAPES[s]
    soln, rhs = (t.cpu().numpy() for t in launch(s, m, mask))
    u, f = reference(s, m, mask)
    eu, ef = max(BT.rel_l2(soln[n], u[n]) for n in range(N)), max(BT.rel_l2(rhs[n], f[n]) for n in range(N))
    print('%s: soln %.3e rhs %.3e (bound %.0e)' % (case_id(case), eu, ef, PER_OP))
    assert eu <= PER_OP and ef <= PER_OP
    outside = np.ones((H, W), dtype=bool)
    outside[BT.unknown_slices(H, W, mask)] = False
    assert np.all(soln[:, outside] == 0.0) and np.all(rhs[:, outside] == 0.0)
    assert np.isfinite(soln).all() and np.isfinite(rhs).all()


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_the_stored_pair_satisfies_the_solvers_operator_to_the_differencing_floor(case):
    """A double(soln) + double(rhs) by pcnn_varcoef_bc_apply: what is left is the float32 rounding of u seen through the stencil - at most
    sum_k m_k beta_k (|du_k| + |du_c|) / dx^2 with |du| <= eps32 / 2 max|u|, i.e. eps32 4 max(beta) max|u| / dx^2 - and the rounding of f itself,
    which is no larger: eps32 * 8 * max(beta) * max|u| / dx^2 per node."""
    from poisson_cnn_amd.dataset import _kernels as K
    s, m, mask = case
    H, W = S.SHAPES[s]
    soln, rhs = launch(s, m, mask)
    rho, rho_h = density(s)
    si, sj = BT.unknown_slices(H, W, mask)
    q, _ = K.varcoef_apply(rho, dev(S.DX), soln.double()[:, si, sj].contiguous(), neumann=B.flags(mask))
    left = (q + rhs.double()[:, si, sj]).abs().amax(dim=(1, 2)).cpu().numpy()
    r64 = rho_h.astype(np.float64)
    beta = np.maximum((2.0 / (r64[:, 1:, :] + r64[:, :-1, :])).max(axis=(1, 2)), (2.0 / (r64[:, :, 1:] + r64[:, :, :-1])).max(axis=(1, 2)))
    bound = S.EPS32 * 8 * beta * soln.abs().amax(dim=(1, 2)).cpu().numpy().astype(np.float64) / np.array(S.DX) ** 2
    print('%s: max|A soln + rhs| %s, floor %s' % (case_id(case), left, bound))
    assert np.all(left <= bound) and np.all(bound > 0)


@pytest.mark.parametrize('case', [c for c in CASES if c[2] in (0, 1, 15)], ids=case_id)
def test_the_solver_returns_the_series_for_its_rhs(case):
    from poisson_cnn_amd import dataset as D
    s, m, mask = case
    H, W = S.SHAPES[s]
    soln, rhs = launch(s, m, mask)
    zeros = {k: torch.zeros((N, W if k in ('left', 'right') else H), device='cuda') for k in B.EDGES}
    back, info = D.variable_density_poisson_solve(density(s)[0], rhs, zeros, dev(S.DX), boundary_types=B.types(mask), return_info=True)
    got = np.array([BT.rel_l2(back[n, 0].cpu().numpy(), soln[n].cpu().numpy()) for n in range(N)])
    fig = round_trip_figure(s, m, mask)
    print('%s: solve against soln %s, twin round trip %s, iterations %s' % (case_id(case), got, fig, info['iterations']))
    assert info['converged'].all()
    assert np.all(got <= 4 * fig)
    if mask == 15:
        shift = np.abs(info['rhs_shift'])
        print('rhs_shift %s' % shift)
        assert np.all(shift <= 1e-6 * rhs.abs().amax(dim=(1, 2)).cpu().numpy())
        assert np.all(info['compatibility_defect'] <= 1e-6)


@pytest.mark.parametrize('mask', [0, 1])
def test_the_flux_form_loss_of_the_pair_is_at_the_solvers_floor(mask):
    from poisson_cnn_amd import configs, dataset as D
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    s, m = 1, 1
    H, W = S.SHAPES[s]
    soln, rhs = launch(s, m, mask)
    rho, d = density(s)[0], dev(np.array(S.DX)[:, None])
    zeros = {k: torch.zeros((N, W if k in ('left', 'right') else H), device='cuda') for k in B.EDGES}
    solved = D.variable_density_poisson_solve(rho, rhs, zeros, d, boundary_types=B.types(mask))
    lossp = dict(configs.hpnn_tiny()['training']['loss_parameters'], mae_loss_weight=0.0, integral_loss_weight=0.0, physics_informed_loss_weight=1.0,
                 physics_informed_loss_config={'stencil_sizes': [3, 3], 'orders': 2, 'normalize': False}, scale_sample_loss_by_target_peak_magnitude=False)
    L = variable_density_loss_wrapper(global_batch_size=N, boundary_types=B.types(mask) if mask else None, **lossp)
    stack = torch.stack([rhs, rho], dim=1)
    own, ref = float(L(soln.view(N, 1, H, W), soln.view(N, 1, H, W), stack, d)), float(L(solved, solved, stack, d))
    print('mask %d: physics term %.4e on the series pair, %.4e on the solver output (mean rhs^2 %.3e)' % (mask, own, ref, float((rhs * rhs).mean())))
    assert np.isfinite(own) and ref > 0 and own <= 2 * ref


def test_launches_are_deterministic_and_independent_of_the_batch():
    from poisson_cnn_amd import ops
    s, m, mask = 2, 1, 6
    H, W = S.SHAPES[s]
    coef, rho, d = dev(S.coefficients(N, *S.MODES[m])), density(s)[0], dev(S.DX)
    a, b = ops.varcoef_series_pair(coef, rho, d, mask), ops.varcoef_series_pair(coef, rho, d, (False, True, True, False))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in range(N):
        one = ops.varcoef_series_pair(coef[n:n + 1].contiguous(), rho[n:n + 1].contiguous(), d[n:n + 1].contiguous(), mask)
        assert torch.equal(one[0][0], a[0][n]) and torch.equal(one[1][0], a[1][n])
    h = ops.handle()
    soln, rhs = torch.full((N, H, W), float('nan'), device='cuda'), torch.full((N, H, W), float('nan'), device='cuda')
    p = lambda t: c_void_p(t.data_ptr())
    h.call('pcnn_varcoef_series_pair', c_int(N), c_int(H), c_int(W), c_int(16), c_int(16), p(coef), c_int(mask), p(rho), p(d), p(soln), p(rhs))
    assert torch.equal(soln, a[0]) and torch.equal(rhs, a[1])                # every node overwritten, NaN nowhere


def test_argument_checks_launch_nothing():
    from poisson_cnn_amd import ops
    h = ops.handle()
    H, W = 9, 11
    coef, rho, d = torch.ones(N, 17, 17, device='cuda'), torch.ones(N, H, W, device='cuda'), torch.full((N,), 0.1, device='cuda')
    soln, rhs = torch.full((N, H, W), 7.0, device='cuda'), torch.full((N, H, W), 7.0, device='cuda')
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else c_void_p(0)

    def call(Hc, Wc, ka, kb, mask, c=coef, r=rho, dd=d, so=soln, rh=rhs):
        return h.lib.pcnn_varcoef_series_pair(h._h, c_int(N), c_int(Hc), c_int(Wc), c_int(ka), c_int(kb), p(c), c_int(mask), p(r), p(dd), p(so), p(rh))
    for kw, word in ((dict(ka=17), 'coefficients'), (dict(kb=0), 'coefficients'), (dict(mask=16), 'neumann_mask'), (dict(mask=-1), 'neumann_mask'),
                     (dict(Hc=2), 'unsupported'), (dict(Wc=2), 'unsupported'), (dict(c=None), 'null'), (dict(r=None), 'null'), (dict(dd=None), 'null'),
                     (dict(so=None), 'null'), (dict(rh=None), 'null')):
        args = dict(dict(Hc=H, Wc=W, ka=4, kb=4, mask=0), **kw)
        assert call(**args) != 0, kw
        text = h.lib.pcnn_last_error(h._h).decode()
        assert 'pcnn_varcoef_series_pair' in text and word in text, text
    torch.cuda.synchronize()
    assert bool((soln == 7.0).all()) and bool((rhs == 7.0).all())
    assert call(H, W, 4, 4, 9) == 0
    torch.cuda.synchronize()
    assert not bool((soln == 7.0).any()) and not bool((rhs == 7.0).any())
    with pytest.raises(ValueError, match='modes'):
        ops.varcoef_series_pair(coef, rho, d)
    with pytest.raises(ValueError, match='neumann_mask'):
        ops.varcoef_series_pair(coef[:, :4, :4].contiguous(), rho, d, 16)
    with pytest.raises(ValueError, match='coef'):
        ops.varcoef_series_pair(coef[:2, :4, :4].contiguous(), rho, d)


# ----------------------------------------------------------------------------- the generator
def generator(**kw):
    from poisson_cnn_amd import dataset as D
    args = dict(batch_size=2, batches_per_epoch=2, fourier_coeff_grid_size_range=(2, 6), output_shape=(33, 47), boundary_types={'left': 'neumann'}, seed=5)
    return D.reverse_variable_density_dataset_generator(**dict(args, **kw))


def test_generator_is_seeded_sharded_and_ordered_as_documented():
    (stack, d), soln = generator()[0]
    (stack2, d2), soln2 = generator()[0]
    assert torch.equal(stack, stack2) and torch.equal(d, d2) and torch.equal(soln, soln2)
    assert tuple(stack.shape) == (2, 2, 33, 47) and tuple(d.shape) == (2, 1) and tuple(soln.shape) == (2, 1, 33, 47)
    assert float(stack[:, 1].min()) >= 1.0 and float(stack[:, 1].max()) <= 10.0
    (stack3, d3), soln3 = generator(shard=(1, 2))[0]
    assert not torch.equal(stack, stack3) and not torch.equal(soln, soln3)
    ref_soln, ref_stack = generator(return_keras_style=False)[0]                  # the reference's order: (soln, stack)
    assert torch.equal(ref_soln, soln) and torch.equal(ref_stack, stack)
    g = generator(output_shape=None, random_output_shape_range=((20, 30), (35, 45)))
    (s4, _), _ = g[0]
    assert 20 <= s4.shape[2] <= 30 and 35 <= s4.shape[3] <= 45 and len(g) == 2
    assert soln[:, 0, -1, :].abs().max() == 0 and soln[:, 0, :, 0].abs().max() == 0 and soln[:, 0, 0, :].abs().max() > 0       # right Dirichlet, left Neumann


@pytest.mark.parametrize('magnitude', [1.0, 3.5])
def test_generator_normalises_rhs_and_the_pair_still_round_trips(magnitude):
    """max|rhs| is the target to one ulp; the scaled pair still solves the equation: the direct fp64 solve of its rhs is the float32-level distance
    from its soln that the twin's recorded figures span (below 100 eps32), and the device solver comes within 4 x that distance."""
    from poisson_cnn_amd import dataset as D
    (stack, d), soln = generator(rhs_max_magnitude=magnitude)[0]
    peak = stack[:, 0].abs().amax(dim=(1, 2)).cpu().numpy()
    assert np.all(np.abs(peak - np.float32(magnitude)) <= np.spacing(np.float32(magnitude)))
    rhs, rho = stack[:, 0].contiguous(), stack[:, 1].contiguous()
    zeros = {k: torch.zeros((2, 47 if k in ('left', 'right') else 33), device='cuda') for k in B.EDGES}
    back = D.variable_density_poisson_solve(rho, rhs, zeros, d, boundary_types={'left': 'neumann'})
    for n in range(2):
        direct = B.solve(rho[n].cpu().numpy().astype(np.float64), rhs[n].cpu().numpy().astype(np.float64), S.zero_edges(33, 47), float(d[n, 0]), 1)
        fig = BT.rel_l2(direct, soln[n, 0].cpu().numpy())
        got = BT.rel_l2(back[n, 0].cpu().numpy(), soln[n, 0].cpu().numpy())
        print('magnitude %g sample %d: direct solve %.3e, device solve %.3e' % (magnitude, n, fig, got))
        assert fig <= 1e2 * S.EPS32 and got <= 4 * fig
    raw = generator(rhs_max_magnitude=None)[0]
    scale = np.float32(magnitude) / raw[0][0][:, 0].abs().amax(dim=(1, 2)).cpu().numpy()
    assert BT.rel_l2(soln[:, 0].cpu().numpy(), raw[1][:, 0].cpu().numpy() * scale[:, None, None]) <= PER_OP        # one factor for both fields


def test_all_neumann_batches_need_no_projection():
    (stack, d), soln = generator(boundary_types={k: 'neumann' for k in B.EDGES}, output_shape=(45, 70))[0]
    w = torch.tensor(S.trapezoid_weights(45, 70), device='cuda')
    for n in range(2):
        assert abs(float((w * soln[n, 0].double()).sum())) <= 45 * 70 * S.EPS32 * float(soln[n].abs().max())       # the float32 rounding of 3150 nodes
        assert abs(float((w * stack[n, 0].double()).sum())) <= 45 * 70 * S.EPS32 * float(stack[n, 0].abs().max())


def test_train_main_runs_two_steps_on_the_analytical_density_dataset(tmp_path, monkeypatch):
    from poisson_cnn_amd import configs, dataset as D, losses, models as M, train
    bt = {'left': 'neumann'}
    cfg = configs.hpnn_tiny()
    cfg['model'].update(density_input=True, postsmoother_iterations=2, boundary_types=bt)
    cfg['dataset'] = {'batch_size': 2, 'batches_per_epoch': 2, 'output_shape': [32, 40], 'fourier_coeff_grid_size_range': [1, 4]}
    cfg['training']['n_epochs'] = 1
    lossp = dict(cfg['training']['loss_parameters'])
    lossp.update(physics_informed_loss_weight=1e-9, mse_loss_weight=0.2, physics_informed_loss_config={'stencil_sizes': [3, 3], 'orders': 2, 'normalize': False})
    cfg['training']['loss_parameters'] = lossp
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    seen = {}
    orig_fit = M.Homogeneous_Poisson_NN_Legacy.fit

    def fit(self, dataset, *a, **kw):
        seen['model'], seen['dataset'], seen['before'] = self, dataset, self.store.flat_w.clone()
        seen['history'] = orig_fit(self, dataset, *a, **kw)
        return seen['history']
    monkeypatch.setattr(M.Homogeneous_Poisson_NN_Legacy, 'fit', fit)
    train.main([str(path), '--dataset_type', 'variable_density_analytical', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    model = seen['model']
    assert isinstance(seen['dataset'], D.reverse_variable_density_dataset_generator) and seen['dataset'].neumann_flags == (True, False, False, False)
    assert model.neumann_mask == 1 and isinstance(model.loss_fn, losses.variable_density_loss_wrapper) and model.loss_fn.neumann_mask == 1
    assert model.optimizer.iterations == 2 and all(np.isfinite(v) for v in seen['history']['loss'])
    assert not torch.equal(model.store.flat_w, seen['before'])
