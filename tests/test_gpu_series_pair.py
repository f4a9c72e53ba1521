"""pcnn_series_pair_synthesis (one launch for a solution / right-hand side pair of a separable series in four per-axis bases), the analytic
generator with a boundary type per edge built on it, and `train.py --dataset_type analytical_mixed`, against the numpy twin of
tests/series_pair_twin.py (whose own properties tests/test_series_pair_reference.py checks without a GPU).

Tolerances: 2e-6 rel-L2 is the project's bound for one float32 operation against fp64 (tests/test_gpu_dataset.py).  Where the mode count is at its
maximum the float32 rounding of the angles omega * t (up to 16 pi) costs more than that whatever evaluates them; there the bound is twice the
error the twin's own float32 restatement reaches against fp64 on the same inputs, computed here, and never below 2e-6."""
import functools
import json
import os
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

from poisson_cnn_amd import configs
from tests import bc_edges_twin as BT
from tests import series_pair_twin as T

pytestmark = pytest.mark.gpu
MIXED = {'left': 'neumann', 'right': 'dirichlet', 'bottom': 'dirichlet', 'top': 'neumann'}
PER_OP = 2e-6


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda')


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def kernel_inputs(N, H, W, ka, kb, ba, bb):
    """float32-representable coefficients and the eigenvalues of realistic spacings for the bases' frequencies; read, never written."""
    rng = np.random.default_rng(H * W + ka)
    c = f32(rng.uniform(-1, 1, (N, ka, kb)))
    dx = rng.uniform(5e-3, 5e-2, N)
    wa = np.arange(1, ka + 1) - (0.5 if ba & 2 else 0.0)
    wb = np.arange(1, kb + 1) - (0.5 if bb & 2 else 0.0)
    return c, f32(T.eigenvalues(wa, dx, H)), f32(T.eigenvalues(wb, dx, W))


def run_pair(c, la, lb, H, W, ba, bb):
    from poisson_cnn_amd.dataset import _kernels as K
    u, f = K.series_pair_synthesis(dev(c), dev(la), dev(lb), H, W, ba, bb)
    return u.cpu().numpy(), f.cpu().numpy()


def check_against_twin(N, H, W, ka, kb, fixed_bound):
    for ba in range(4):
        for bb in range(4):
            c, la, lb = kernel_inputs(N, H, W, ka, kb, ba, bb)
            u, f = run_pair(c, la, lb, H, W, ba, bb)
            ru, rf = T.pair(c, la, lb, H, W, ba, bb)
            if fixed_bound is not None:
                bu = bf = fixed_bound
            else:
                u32, f32_ = T.pair(c, la, lb, H, W, ba, bb, dtype=np.float32)
                bu, bf = max(PER_OP, 2 * rel(u32, ru)), max(PER_OP, 2 * rel(f32_, rf))
            eu, ef = rel(u, ru), rel(f, rf)
            print('%dx%d, %dx%d modes, bases %d,%d: soln %.3g (bound %.3g)  rhs %.3g (bound %.3g)' % (H, W, ka, kb, ba, bb, eu, bu, ef, bf))
            assert u.shape == (N, H, W) and f.shape == (N, H, W)
            assert eu <= bu and ef <= bf, (ba, bb, eu, bu, ef, bf)


def test_kernel_at_the_series_test_shape():
    check_against_twin(3, 45, 70, 5, 8, PER_OP)


def test_kernel_at_the_maximum_mode_count_on_a_grid_narrower_than_a_wave():
    check_against_twin(3, 33, 17, 16, 16, None)


def test_kernel_over_several_column_tiles():
    """W = two full column tiles and a remainder, H = 17 = less than one row tile and not a multiple of the rows a thread keeps."""
    from poisson_cnn_amd.dataset import _kernels as K
    rows, cols = K.SERIES_PAIR_TILE
    assert 17 < rows
    check_against_twin(3, 17, 2 * cols + 37, 5, 8, None)


def test_kernel_over_several_row_tiles():
    from poisson_cnn_amd.dataset import _kernels as K
    rows, cols = K.SERIES_PAIR_TILE
    check_against_twin(3, 2 * rows + rows // 2 + 3, cols + 1, 3, 2, None)


def test_zero_eigenvalues_give_a_zero_right_hand_side():
    c, la, lb = kernel_inputs(3, 45, 70, 5, 8, 2, 3)
    u, f = run_pair(c, np.zeros_like(la), np.zeros_like(lb), 45, 70, 2, 3)
    assert np.abs(u).max() > 0 and not f.any()


def test_no_width_refusal():
    from poisson_cnn_amd.dataset import _kernels as K
    N, H, W, ka, kb = 1, 16, 4099, 16, 4
    c, la, lb = kernel_inputs(N, H, W, ka, kb, 2, 0)
    with pytest.raises(RuntimeError, match='too wide'):
        K.series_synthesis(dev(c), H, W, 0)
    u, f = run_pair(c, la, lb, H, W, 2, 0)
    ru, rf = T.pair(c, la, lb, H, W, 2, 0)
    u32, f32_ = T.pair(c, la, lb, H, W, 2, 0, dtype=np.float32)
    eu, ef, bu, bf = rel(u, ru), rel(f, rf), max(PER_OP, 2 * rel(u32, ru)), max(PER_OP, 2 * rel(f32_, rf))
    print('16x4099, 16x4 modes: soln %.3g (bound %.3g)  rhs %.3g (bound %.3g)' % (eu, bu, ef, bf))
    assert eu <= bu and ef <= bf


def test_argument_checks_launch_nothing():
    from poisson_cnn_amd import ops
    h = ops.handle()
    N, H, W = 2, 9, 11
    coef, lam = torch.ones(N, 17, 17, device='cuda'), torch.ones(N, 17, device='cuda')
    soln, rhs = torch.full((N, H, W), 7.0, device='cuda'), torch.full((N, H, W), 7.0, device='cuda')
    p = lambda t: c_void_p(t.data_ptr())

    def call(ka, kb, basis_a, basis_b, out_soln, out_rhs):
        return h.lib.pcnn_series_pair_synthesis(h._h, c_int(N), c_int(H), c_int(W), c_int(ka), c_int(kb), p(coef), p(lam), p(lam), c_int(basis_a),
                                                c_int(basis_b), out_soln, out_rhs)
    for args, word in (((4, 4, 4, 0, p(soln), p(rhs)), 'basis'), ((4, 4, 0, -1, p(soln), p(rhs)), 'basis'), ((17, 4, 0, 0, p(soln), p(rhs)), 'coefficients'),
                       ((4, 17, 0, 0, p(soln), p(rhs)), 'coefficients'), ((4, 4, 0, 0, p(soln), c_void_p(0)), 'null'), ((4, 4, 0, 0, None, p(rhs)), 'null')):
        assert call(*args) != 0
        text = h.lib.pcnn_last_error(h._h).decode()
        assert 'pcnn_series_pair_synthesis' in text and word in text, text
    torch.cuda.synchronize()
    assert bool((soln == 7.0).all()) and bool((rhs == 7.0).all())
    assert call(4, 4, 3, 2, p(soln), p(rhs)) == 0
    torch.cuda.synchronize()
    assert not bool((soln == 7.0).any()) and not bool((rhs == 7.0).any())
    from poisson_cnn_amd.dataset import _kernels as K
    with pytest.raises(ValueError):
        K.series_pair_synthesis(coef[:, :4, :4].contiguous(), lam[:, :3].contiguous(), lam[:, :4].contiguous(), H, W, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- the generator
def analytic_cfg(**kw):
    """configs.hpnn()'s dataset section narrowed to a batch of 3 on [120, 160]^2, without the keys the Dirichlet generator alone reads."""
    cfg = dict(configs.hpnn()['dataset'])
    for k in ('taylor_degree_range', 'homogeneous_bc', 'return_boundaries'):
        cfg.pop(k)
    cfg.update(batch_size=3, random_output_shape_range=[[120, 160], [120, 160]])
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize('name', ['dirichlet', 'neumann'])
def test_uniform_flags_reproduce_the_sibling_generator(name):
    from poisson_cnn_amd.dataset import (reverse_poisson_dataset_generator, reverse_poisson_dataset_generator_homogeneous_neumann,
                                         reverse_poisson_dataset_generator_mixed)
    cfg = analytic_cfg()
    if name == 'dirichlet':
        sibling = reverse_poisson_dataset_generator(seed=4, homogeneous_bc=True, taylor_degree_range=None, return_boundaries=False, **cfg)
    else:
        sibling = reverse_poisson_dataset_generator_homogeneous_neumann(seed=4, **cfg)
    mixed = reverse_poisson_dataset_generator_mixed(seed=4, boundary_types={e: name for e in T.EDGES}, **cfg)
    assert len(mixed) == len(sibling) == cfg['batches_per_epoch']
    for _ in range(2):                                            # the second batch too: both consumed the same draws for the first
        (rhs_s, dx_s), soln_s = sibling[0]
        (rhs_m, dx_m), soln_m = mixed[0]
        assert rhs_m.shape == rhs_s.shape and soln_m.shape == soln_s.shape and torch.equal(dx_m, dx_s)
        er, es = rel(rhs_m.cpu().numpy(), rhs_s.cpu().numpy()), rel(soln_m.cpu().numpy(), soln_s.cpu().numpy())
        print('%s: rhs %.3g, soln %.3g against the sibling generator' % (name, er, es))
        assert er <= 2 * PER_OP and es <= 2 * PER_OP             # each side within the per-operation bound of the exact pair


@pytest.mark.parametrize('types', [{'left': 'neumann', 'top': 'neumann'}, {'right': 'neumann'}, {'left': 'neumann', 'right': 'neumann', 'bottom': 'neumann'}],
                         ids=['left+top', 'right', 'left+right+bottom'])
def test_generated_pairs_solve_the_pde_with_their_edge_conditions(types):
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator_mixed
    gen = reverse_poisson_dataset_generator_mixed(seed=6, boundary_types=types, **analytic_cfg(normalizations=None, fourier_coeff_grid_size_range=[[1, 4], [1, 4]]))
    assert gen.neumann_flags == T.neumann_flags(types)
    (rhs, dx), soln = gen[0]
    u, f, h = soln.cpu().numpy().astype(np.float64)[:, 0], rhs.cpu().numpy().astype(np.float64)[:, 0], dx.cpu().numpy().astype(np.float64)[:, 0]
    res = T.pde_residual(u, f, h)
    dirichlet, neumann = T.edge_defects(u, gen.neumann_flags)
    print('%s on %s: PDE rel-L2 %.3g, Dirichlet edges %.3g, Neumann edges %.3g' % (types, u.shape, res, dirichlet, neumann))
    assert res <= 5e-2 and dirichlet <= 1e-5 and neumann <= 5e-3


def test_generator_outputs_normalisation_shards_and_bad_edges():
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator, reverse_poisson_dataset_generator_mixed
    gen = reverse_poisson_dataset_generator_mixed(seed=2, boundary_types=MIXED, **analytic_cfg())
    assert isinstance(gen, reverse_poisson_dataset_generator) and gen.neumann_flags == (True, False, False, True)
    inp, soln = gen[0]
    assert len(inp) == 2 and soln.dim() == 4 and soln.shape[:2] == (3, 1) and 120 <= soln.shape[2] <= 160 and 120 <= soln.shape[3] <= 160
    assert inp[0].shape == soln.shape and inp[1].shape == (3, 1) and inp[0].dtype == soln.dtype == torch.float32 and soln.is_cuda
    assert np.allclose(inp[0].abs().amax(dim=(1, 2, 3)).cpu().numpy(), 1.0, rtol=1e-6)
    inp, soln = reverse_poisson_dataset_generator_mixed(seed=2, boundary_types=MIXED, **analytic_cfg(return_dx=False, return_rhses=True))[0]
    assert len(inp) == 1 and inp[0].shape == soln.shape
    gen.fixed_output_shape = (64, 80)
    assert gen[0][1].shape == (3, 1, 64, 80)
    a = reverse_poisson_dataset_generator_mixed(seed=2, boundary_types=MIXED, shard=(0, 2), **analytic_cfg())
    b = reverse_poisson_dataset_generator_mixed(seed=2, boundary_types=MIXED, shard=(1, 2), **analytic_cfg())
    for _ in range(2):
        ya, yb = a[0][1], b[0][1]
        assert ya.shape == yb.shape and not torch.equal(ya, yb)
    for bad in ({'front': 'neumann'}, {'left': 'robin'}):
        with pytest.raises(ValueError, match='boundary_types'):
            reverse_poisson_dataset_generator_mixed(boundary_types=bad, **analytic_cfg())


# ---------------------------------------------------------------------------------------------------------------- training
def test_one_train_step_on_a_generated_batch():
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator_mixed
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    from poisson_cnn_amd.train import Adam
    full = configs.hpnn_tiny()
    gen = reverse_poisson_dataset_generator_mixed(seed=3, boundary_types=MIXED, **analytic_cfg(batch_size=2))
    gen.fixed_output_shape = (64, 64)
    inp, soln = gen[0]
    assert soln.shape == (2, 1, 64, 64)
    model = Homogeneous_Poisson_NN_Legacy(**dict(full['model'], bc_type=MIXED, postsmoother_iterations=2, smoother_boundaries='enforce'))
    model.compile(loss=loss_wrapper(global_batch_size=2, **full['training']['loss_parameters']), optimizer=Adam(learning_rate=1e-5))
    logs = model.train_step((inp, soln))
    assert np.isfinite(float(logs['loss'])) and float(model.store.flat_g.abs().max()) > 0


def _train_config(bc_type=MIXED):
    cfg = configs.hpnn_tiny()
    cfg['model'].update(bc_type=bc_type, postsmoother_iterations=2, smoother_boundaries='enforce')
    cfg['dataset'] = analytic_cfg(batch_size=2, batches_per_epoch=2, random_output_shape_range=[[64, 72], [64, 72]])
    cfg['training']['n_epochs'] = 1
    return cfg


def test_train_main_with_the_analytic_mixed_dataset(tmp_path, monkeypatch):
    from poisson_cnn_amd import models as M, train
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator_mixed
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(_train_config()))
    seen = {}
    orig_fit = M.Homogeneous_Poisson_NN_Legacy.fit

    def fit(self, dataset, *a, **kw):
        seen['model'], seen['dataset'] = self, dataset
        seen['history'] = orig_fit(self, dataset, *a, **kw)
        return seen['history']
    monkeypatch.setattr(M.Homogeneous_Poisson_NN_Legacy, 'fit', fit)
    train.main([str(path), '--dataset_type', 'analytical_mixed', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    assert type(seen['dataset']) is reverse_poisson_dataset_generator_mixed
    assert list(seen['dataset'].neumann_flags) == BT.bits(seen['model'].neumann_mask) and seen['model'].neumann_mask == BT.mask_of(MIXED)
    assert all(np.isfinite(v) for v in seen['history']['loss']) and len(seen['history']['loss']) == 1
    assert any(f.startswith('chkpt') for f in os.listdir(tmp_path))


def test_train_main_refuses_the_option_elsewhere(tmp_path):
    from poisson_cnn_amd import train
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(_train_config(bc_type='neumann')))
    with pytest.raises(ValueError, match='--dataset_type analytical_mixed'):
        train.main([str(path), '--dataset_type', 'analytical_mixed', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    path.write_text(json.dumps(_train_config()))
    with pytest.raises(ValueError, match='--dataset_type analytical_mixed'):
        train.main([str(path), '--dataset_type', 'analytical_mixed', '--model', 'unet', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
