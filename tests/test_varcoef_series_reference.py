"""The fp64 twin of pcnn_varcoef_series_pair (tests/varcoef_series_twin.py) against the sparse system of
tests/varcoef_bc_twin.py, the properties the solve-free generator rests on, the noise argument that asks for the fused kernel, and the host-side
refusals of reverse_variable_density_dataset_generator and train.py.  No GPU."""
import hashlib
import json

import numpy as np
import pytest

from tests import varcoef_bc_twin as B, varcoef_series_twin as S, varcoef_train_bc_twin as BT

H, W = 9, 12


def small(mask, seed=3):
    rng = np.random.default_rng([seed, mask])
    coef = 2 * rng.uniform(size=(1, 3, 4)) - 1
    rho = rng.uniform(1.0, 10.0, (1, H, W))
    dx = np.array([0.037])
    return coef, rho, dx


def unknowns_of(a, mask):
    si, sj = BT.unknown_slices(a.shape[-2], a.shape[-1], mask)
    return a[..., si, sj]


@pytest.mark.parametrize('mask', range(16))
def test_rhs_is_minus_the_sparse_operator_on_the_unknowns(mask):
    coef, rho, dx = small(mask)
    u, f = S.twin(coef, rho, dx, mask)
    A, _ = B.assemble(rho[0], dx[0], mask)
    want = -(A @ unknowns_of(u[0], mask).ravel())
    assert np.abs(unknowns_of(f[0], mask).ravel() - want).max() <= 1e-12 * np.abs(want).max()
    outside = np.ones((H, W), dtype=bool)
    outside[BT.unknown_slices(H, W, mask)] = False
    assert np.all(u[0][outside] == 0.0) and np.all(f[0][outside] == 0.0)                    # exact zeros on the Dirichlet nodes


def test_all_neumann_pair_has_zero_trapezoid_sums():
    """Cosine modes A >= 1 sum to zero under the trapezoid rule, and sum w L u = u^T (W A) 1 = 0: no projection, no rhs_shift."""
    for shape in ((H, W), (33, 47)):
        coef = S.coefficients(1, 5, 8)
        rho = S.density(S.smooth_unit_field(1, *shape))
        u, f = S.twin(coef, rho, np.array([0.02]), 15)
        w = S.trapezoid_weights(*shape)
        assert abs((w * u[0]).sum()) <= 1e-13 * np.abs(u[0]).max()
        assert abs((w * f[0]).sum()) <= 1e-13 * np.abs(f[0]).max()


@pytest.mark.parametrize('mask', range(16))
def test_direct_solve_of_the_rhs_gives_the_series_back(mask):
    coef, rho, dx = small(mask)
    u, f = S.twin(coef, rho, dx, mask)
    back = B.solve(rho[0], f[0], S.zero_edges(H, W), dx[0], mask)               # mask 15: the projected system, zero w-mean
    assert BT.rel_l2(unknowns_of(back, mask), unknowns_of(u[0], mask)) <= 1e-9


def analytic_pair(n, mask):
    """One mode on the unit square (dx = 1 / (n - 1), so t = pi x): u = phi(x) psi(y) and div((1/rho) grad u) for rho = 1 + x + 0.5 y."""
    ka, kb = 2, 1
    ba, bb, wa, wb = S.SP.bases_of(B.flags(mask), ka, kb)
    x, y = np.linspace(0.0, 1.0, n)[:, None], np.linspace(0.0, 1.0, n)[None, :]
    fa, fb = np.pi * wa[ka - 1], np.pi * wb[kb - 1]
    trig = lambda kind, t: np.cos(t) if kind & 1 else np.sin(t)
    dtrig = lambda kind, t: -np.sin(t) if kind & 1 else np.cos(t)
    rho = 1.0 + x + 0.5 * y
    lap = -(fa ** 2 + fb ** 2) * trig(ba, fa * x) * trig(bb, fb * y)
    ux, uy = fa * dtrig(ba, fa * x) * trig(bb, fb * y), fb * trig(ba, fa * x) * dtrig(bb, fb * y)
    coef = np.zeros((1, ka, kb))
    coef[0, ka - 1, kb - 1] = 1.0
    return coef, rho[None], np.array([1.0 / (n - 1)]), lap / rho - (1.0 * ux + 0.5 * uy) / rho ** 2


@pytest.mark.parametrize('mask', [0, 9])
def test_the_discrete_rhs_is_second_order(mask):
    """Away from Neumann edges: on such an edge's nodes the doubled inward face stands for the half cell's two faces and f there is first-order
    consistent (the SOLVE stays second order), so those lines are left out of the norm."""
    errs = []
    for n in (33, 65):
        coef, rho, dx, exact = analytic_pair(n, mask)
        _, f = S.twin(coef, rho, dx, mask)
        errs.append(np.abs(f[0] - exact)[1:-1, 1:-1].max())
    print('mask %d: max error %.3e at 33^2, %.3e at 65^2, ratio %.2f' % (mask, errs[0], errs[1], errs[0] / errs[1]))
    assert 3.6 <= errs[0] / errs[1] <= 4.4


def test_differencing_a_rounded_solution_is_what_the_fused_kernel_avoids():
    """97 x 65, the (1,1) mode only: the operator applied to float32(u) is off by eps32 4 n^2 / (pi k)^2 in grid-scale noise; rounding f itself
    costs half an ulp per node."""
    Hn, Wn = S.SHAPES[2]
    coef = np.zeros((1, 1, 1))
    coef[0, 0, 0] = 1.0
    rho = S.density(S.smooth_unit_field(1, Hn, Wn), 1.0, 10.0).astype(np.float64)
    dx = np.array([0.01])
    u, f = S.twin(coef, rho, dx, 0)
    A, _ = B.assemble(rho[0], dx[0], 0)
    noisy = -(A @ unknowns_of(u[0].astype(np.float32).astype(np.float64), 0).ravel())
    exact = unknowns_of(f[0], 0).ravel()
    routed, rounded = BT.rel_l2(noisy, exact), BT.rel_l2(exact.astype(np.float32), exact)
    print('97 x 65, mode (1,1): operator on float32(u) %.3e rel-L2, float32(f) %.3e; estimate eps32 4 n^2 / (pi k)^2 = %.1e'
          % (routed, rounded, S.EPS32 * 4 * Hn ** 2 / np.pi ** 2))
    assert routed > 1e-5 and rounded < 1e-7


@pytest.mark.parametrize('shape', S.SHAPES, ids=lambda s: '%dx%d' % s)
def test_round_trip_figure_of_the_stored_pair(shape):
    """The figure the GPU round trip is held to (4 x, tests/test_gpu_varcoef_series.py): ratio 1000, both mode sets, masks 0 / 1 / 15.  It is the two
    float32 roundings seen through A^-1, so it sits at the float32 level: above a hundredth of an ulp, below a hundred."""
    rho = S.density(S.smooth_unit_field(3, *shape))
    for modes in S.MODES:
        for mask in (0, 1, 15):
            fig = S.round_trip(S.coefficients(3, *modes), rho, S.DX, mask)
            print('%d x %d, %d x %d modes, mask %2d: round trip rel-L2 %s' % (shape + modes + (mask,) + (' '.join('%.2e' % v for v in fig),)))
            assert np.all(fig > 1e-2 * S.EPS32) and np.all(fig < 1e2 * S.EPS32)


# ----------------------------------------------------------------------------- host-side refusals
def test_generator_refuses_bad_arguments_without_a_device():
    from poisson_cnn_amd import dataset as D
    G = D.reverse_variable_density_dataset_generator
    ok = dict(batch_size=2, batches_per_epoch=1, fourier_coeff_grid_size_range=(1, 8), device='cpu')
    assert len(G(**ok)) == 1 and G(**dict(ok, boundary_types={'left': 'neumann'})).neumann_flags == (True, False, False, False)
    with pytest.raises(ValueError, match='density_profile'):
        G(**dict(ok, density_profile='linear'))
    with pytest.raises(ValueError, match='density_range'):
        G(**dict(ok, density_range=(0.0, 10.0)))
    with pytest.raises(ValueError, match='density_range'):
        G(**dict(ok, density_range=(5.0, 1.0)))
    with pytest.raises(ValueError, match='density_smoothness_range'):
        G(**dict(ok, density_smoothness_range=(1, 20)))
    with pytest.raises(ValueError, match='boundary_types'):
        G(**dict(ok, boundary_types={'left': 'robin'}))
    with pytest.raises(ValueError, match='boundary_types'):
        G(**dict(ok, boundary_types={'front': 'neumann'}))
    with pytest.raises(ValueError, match='fourier_coeff_grid_size_range'):
        G(**dict(ok, fourier_coeff_grid_size_range=(1, 17)))
    with pytest.raises(ValueError, match='fourier_coeff_grid_size_range'):
        G(**dict(ok, fourier_coeff_grid_size_range=(16, 16)))               # lo == hi draws lo + 1 modes
    with pytest.raises(ValueError, match='fourier_coeff_grid_size_range'):
        G(**dict(ok, fourier_coeff_grid_size_range=(4, 2)))
    G(**dict(ok, fourier_coeff_grid_size_range=(15, 15)))
    G(**dict(ok, fourier_coeff_grid_size_range=((1, 16), (0, 3))))
    with pytest.raises(ValueError, match='output_shape'):
        G(**dict(ok, output_shape=(2, 40)))
    with pytest.raises(ValueError, match='random_dx_range'):
        G(**dict(ok, random_dx_range=(0.0, 0.05)))
    with pytest.raises(ValueError, match='rhs_max_magnitude'):
        G(**dict(ok, rhs_max_magnitude=0.0))
    with pytest.raises(ValueError, match='shard'):
        G(**dict(ok, shard=(2, 2)))
    # the sibling words the shared refusals the same way
    for kw in (dict(density_profile='linear'), dict(density_range=(0.0, 10.0)), dict(density_smoothness_range=(1, 20))):
        texts = []
        for cls in (G, D.variable_density_dataset_generator):
            with pytest.raises(ValueError) as e:
                cls(**dict(dict(batch_size=2, device='cpu'), **kw))
            texts.append(str(e.value))
        assert texts[0] == texts[1]


def _config(tmp_path, **model):
    from poisson_cnn_amd import configs
    cfg = configs.hpnn_tiny()
    cfg['model'].update(postsmoother_iterations=2, **model)
    cfg['dataset'] = {'batch_size': 2, 'batches_per_epoch': 2, 'output_shape': [32, 40], 'fourier_coeff_grid_size_range': [1, 4]}
    cfg['training']['n_epochs'] = 1
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    return cfg, path


@pytest.mark.parametrize('dataset_type', ['variable_density', 'variable_density_analytical'])
def test_train_refuses_inconsistent_sections_for_both_density_dataset_types(tmp_path, dataset_type):
    from poisson_cnn_amd import train
    run = lambda path, dt=dataset_type, *more: train.main([str(path), '--dataset_type', dt, '--checkpoint_dir', str(tmp_path), '--epochs', '1'] + list(more))
    cfg, path = _config(tmp_path)                                            # no density_input in the model section
    with pytest.raises(ValueError, match='--dataset_type %s yields' % dataset_type):
        run(path)
    cfg, path = _config(tmp_path, density_input=True)
    with pytest.raises(ValueError, match='--dataset_type %s yields' % dataset_type):
        run(path, dataset_type, '--model', 'unet')
    for other in ('analytical', 'numerical', 'analytical_mixed'):            # the density model takes both density dataset types and no other
        with pytest.raises(ValueError, match='density_input'):
            run(path, other)
    cfg['dataset']['boundaries'] = 'random'
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="--dataset_type %s trains the homogeneous model: it needs boundaries 'zero'" % dataset_type):
        run(path)
    del cfg['dataset']['boundaries']
    cfg['dataset']['boundary_types'] = {'left': 'neumann'}                   # Neumann in the dataset section alone
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match='--dataset_type %s with Neumann boundary_types' % dataset_type):
        run(path)
    cfg['model']['boundary_types'] = {'top': 'neumann'}                      # the two sections disagree
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match='--dataset_type %s: the model section has boundary_types' % dataset_type):
        run(path)
    cfg['model']['boundary_types'] = 'neumann'
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="dict edge -> 'dirichlet'"):
        run(path)
    with pytest.raises(ValueError, match='Invalid dataset type'):
        run(path, 'variable_density_reverse')


def test_the_entry_point_is_declared_and_bound_from_the_header():
    from poisson_cnn_amd import _lib
    protos = _lib.header_prototypes()
    assert protos.get('pcnn_varcoef_series_pair') == ('int', ['pcnn_handle'] + ['int'] * 5 + ['const float*', 'int', 'const float*', 'const float*', 'float*', 'float*'])


# ----------------------------------------------------------------------------- the solver-made generator's draws and launches are untouched
class _Recorder:
    """Stands in for dataset._kernels: every call is logged by name with a digest of its array arguments, and answers with host tensors."""

    def __init__(self):
        self.log = []

    def _note(self, name, *args):
        import torch
        h = hashlib.sha256()
        for a in args:
            if isinstance(a, torch.Tensor):
                h.update(np.ascontiguousarray(a.numpy()).tobytes())
                h.update(repr(tuple(a.shape)).encode())
            else:
                h.update(repr(a).encode())
        self.log.append((name, h.hexdigest()[:16]))

    def resize_legacy_bicubic(self, x, out_hw):
        import torch
        self._note('resize', x, tuple(out_hw))
        return torch.zeros((x.shape[0], out_hw[0], out_hw[1], 1), dtype=torch.float32) + x.reshape(x.shape[0], -1)[:, :1].reshape(-1, 1, 1, 1)

    def set_max_magnitude(self, x, target):
        self._note('set_max_magnitude', x, target)
        return target

    def varcoef_density(self, g, lo, hi):
        self._note('density', g, lo, hi)
        return g

    def varcoef_density_smooth(self, g, lo, hi):
        self._note('density_smooth', g, lo, hi)
        return g


# the digest of the parent commit's call stream for the arguments below (recorded by running this very test body on it)
SOLVER_GENERATOR_STREAM = {'abs': '17d40b9895a88e4b521cc89d24567f6a33925637e991c497ed769fd8ca72eb5d',
                           'smooth': '0106bb30e45b145f4d012c615a5f27011aaebb5cdfb9e2f7b6639edbd20fa8f7'}


def _solver_generator_stream(monkeypatch, profile):
    import torch
    from poisson_cnn_amd import dataset as D
    rec = _Recorder()
    monkeypatch.setattr(D, 'K', rec)
    seen = {}

    def solve(rho, rhs, bc, d, **kw):
        rec._note('solve', rho, rhs, d, *[bc[k] for k in sorted(bc)], sorted((k, repr(v)) for k, v in kw.items()))
        seen['kw'] = kw
        info = {k: np.zeros(rho.shape[0]) for k in ('iterations', 'converged', 'relative_residual', 'compatibility_defect', 'rhs_shift')}
        return torch.zeros((rho.shape[0], 1) + tuple(rho.shape[1:])), info
    monkeypatch.setattr(D, 'variable_density_poisson_solve', solve)
    gen = D.variable_density_dataset_generator(batch_size=3, batches_per_epoch=2, seed=11, device='cpu', density_profile=profile, density_range=(1.0, 100.0),
                                               boundaries='random', boundary_types={'left': 'neumann'})
    for _ in range(2):
        (stack, *edges, d), soln = gen[0]
        assert tuple(stack.shape[:2]) == (3, 2) and len(edges) == 4
    return hashlib.sha256(repr(rec.log).encode()).hexdigest()


@pytest.mark.parametrize('profile', ['abs', 'smooth'])
def test_solver_made_generator_draws_and_launches_what_it_did(monkeypatch, profile):
    """variable_density_dataset_generator(seed=s)[0] is unchanged by the helpers it now shares: the same draws in the same order reach the same
    kernels with the same arguments (two batches, random edges, a Neumann edge), by the digest recorded on the parent commit."""
    got = _solver_generator_stream(monkeypatch, profile)
    print(profile, got)
    assert got == SOLVER_GENERATOR_STREAM[profile]
