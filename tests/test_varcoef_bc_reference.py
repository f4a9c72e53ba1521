"""The numpy / scipy twin of the variable-density solve with per-edge Dirichlet / Neumann boundaries (tests/varcoef_bc_twin.py) has the properties the
device code of poisson_cnn_amd/csrc/varcoef.hip rests on, and the Python entry point refuses bad boundary types before it
touches a device - no GPU needed."""
import functools

import numpy as np
import pytest
import scipy.linalg

from tests import varcoef_bc_twin as B
from tests import varcoef_twin as T

EDGES = B.EDGES
MASKS = list(range(16))


@functools.lru_cache(maxsize=None)
def problem(H, W, ratio=10.0, seed=0):
    rng = np.random.default_rng(seed + 1000 * H + W)
    rho = T.smooth_density(rng, H, W, 1.0, ratio)
    f = rng.uniform(-1, 1, (H, W))
    e = {k: rng.uniform(-1, 1, W if k in ('left', 'right') else H) for k in EDGES}
    return rho, f, e, 0.03


@functools.lru_cache(maxsize=None)
def system(H, W, mask, ratio=10.0):
    rho, f, e, dx = problem(H, W, ratio)
    A, b = B.assemble(rho, dx, mask, e, f)
    return A, b, B.weights(H, W, mask).ravel()


@pytest.mark.parametrize('mask', MASKS)
def test_weighted_matrix_is_symmetric_and_definite(mask):
    """W A symmetric to rounding; positive definite with a Dirichlet edge; mask 15: semi-definite, null space = the constants, sum w (A u) = 0."""
    H, W = 7, 9
    A, _, w = system(H, W, mask)
    WA = w[:, None] * A.toarray()
    assert np.abs(WA - WA.T).max() <= 1e-12 * np.abs(WA).max()
    ev = np.linalg.eigvalsh(0.5 * (WA + WA.T))
    if mask != 15:
        assert ev.min() > 0.0
        return
    scale = ev.max()
    assert abs(ev[0]) <= 1e-12 * scale and ev[1] > 1e-6 * scale            # one null direction ...
    assert np.abs(A @ np.ones(A.shape[0])).max() <= 1e-12 * np.abs(A).max() * 5      # ... the constants
    u = np.random.default_rng(1).standard_normal(A.shape[0])
    assert abs(w @ (A @ u)) <= 1e-12 * np.abs(w * (A @ u)).sum()


@pytest.mark.parametrize('mask', MASKS)
def test_constant_density_is_the_constant_coefficient_operator(mask):
    """rho = c: A = M / (c h^2) with M the operator of pcnn_fd_poisson_mixed, so the system is mixed_bc_poisson_solve's with c f for f."""
    H, W, c, dx = 6, 8, 2.5, 0.03
    A, _ = B.assemble(np.full((H, W), c), dx, mask)
    M = B.constant_operator(H, W, mask)
    assert np.abs(A.toarray() - M / (c * dx * dx)).max() <= 1e-12 * np.abs(A).max()


def test_constant_density_right_hand_side_is_the_mixed_solver_s():
    """... and b = (mixed solver's right-hand side with c f) / (c h^2): -h^2 c f + Dirichlet neighbours + 2 h g, against oracle.dataset's solve."""
    from oracle import dataset as ods
    H, W, c = 9, 12, 2.5
    _, f, e, dx = problem(H, W)
    for mask in (5, 7, 10):
        ref = ods.mixed_bc_poisson_solve(c * f[None], {k: v[None] for k, v in e.items()}, np.array([dx]), dict(zip(EDGES, B.flags(mask))))[0]
        got = B.solve(np.full((H, W), c), f, e, dx, mask)
        assert np.linalg.norm(got - ref) <= 1e-10 * np.linalg.norm(ref)


def test_mask_0_is_the_dirichlet_twin_exactly():
    H, W = 9, 11
    rho, f, e, dx = problem(H, W)
    A, b = B.assemble(rho, dx, 0, e, f)
    A0, b0 = T.assemble(rho, dx), T.right_hand_side(rho, f, e, dx)
    assert abs(A - A0).max() == 0.0 and np.array_equal(b, b0)
    assert np.array_equal(B.embed(np.zeros((H - 2) * (W - 2)), e, H, W, 0), T.embed(np.zeros((H - 2) * (W - 2)), e, H, W))


@pytest.mark.parametrize('mask', MASKS)
def test_generalised_eigenvalues_lie_between_the_face_coefficients(mask):
    """(W A) v = mu (W M / h^2) v: mu in [min beta, max beta], so the preconditioned condition number is at most max(beta) / min(beta)."""
    H, W = 7, 9
    rho, _, _, dx = problem(H, W)
    A, _, w = system(H, W, mask)
    WA = w[:, None] * A.toarray()
    WM = w[:, None] * B.constant_operator(H, W, mask) / dx ** 2
    WA, WM = 0.5 * (WA + WA.T), 0.5 * (WM + WM.T)
    if mask == 15:                                                         # on the complement of the common null space
        Q = scipy.linalg.null_space(np.ones((1, WA.shape[0])))
        WA, WM = Q.T @ WA @ Q, Q.T @ WM @ Q
    mu = scipy.linalg.eigh(WA, WM, eigvals_only=True)
    bi, bj = T.face_coefficients(rho)
    lo, hi = min(bi.min(), bj.min()), max(bi.max(), bj.max())
    assert lo - 1e-9 <= mu.min() and mu.max() <= hi + 1e-9


@pytest.mark.parametrize('mask', [5, 10, 15])
@pytest.mark.parametrize('H,W', [(7, 9), (19, 70)])
def test_weighted_pcg_agrees_with_the_direct_solve(mask, H, W):
    rho, f, e, dx = problem(H, W)
    A, b, _ = system(H, W, mask)
    x, it, rel = B.pcg(A, b, H, W, mask, tol=1e-10)
    direct = B.solve(rho, f, e, dx, mask)
    got = B.embed(x, e, H, W, mask)
    err = np.linalg.norm(got - direct) / np.linalg.norm(direct)
    print('mask %d %dx%d: %d iterations, residual %.2e, error %.2e' % (mask, H, W, it, rel, err))
    assert rel <= 1e-10 and err <= 1e-9 and it <= 40


def test_mask_15_projection_and_mean():
    H, W = 7, 9
    rho, f, e, dx = problem(H, W)
    A, b, w = system(H, W, 15)
    bp, defect, m = B.project(b, B.weights(H, W, 15))
    assert 0.0 < defect <= 1.0 and abs(w @ bp) <= 1e-12 * np.abs(w * bp).sum()
    u = B.solve(rho, f, e, dx, 15).ravel()
    assert abs(w @ u) <= 1e-12 * np.abs(w * u).sum()                       # zero trapezoidal integral
    assert np.abs(A @ u - bp).max() <= 1e-9 * np.abs(bp).max()             # and it solves the projected system
    # shifting f by the constant the projection took off b reproduces the projected right-hand side
    _, b_shifted = B.assemble(rho, dx, 15, e, f + m)
    assert np.abs(b_shifted - bp).max() <= 1e-12 * np.abs(bp).max()


# ----------------------------------------------------------------------------- host-side argument checks of the Python entry point
def solve_args(N=2, H=9, W=11):
    rho = np.ones((N, H, W), dtype=np.float32)
    f = np.zeros((N, 1, H, W), dtype=np.float32)
    b = {k: np.zeros((N, W if k in ('left', 'right') else H), dtype=np.float32) for k in EDGES}
    return rho, f, b, np.full((N, 1), 0.01, dtype=np.float32)


def test_entry_point_refuses_bad_boundary_types_without_a_device():
    from poisson_cnn_amd import dataset as D
    rho, f, b, dx = solve_args()
    with pytest.raises(ValueError, match='front'):
        D.variable_density_poisson_solve(rho, f, b, dx, boundary_types={'front': 'neumann'})
    with pytest.raises(ValueError, match='robin'):
        D.variable_density_poisson_solve(rho, f, b, dx, boundary_types={'left': 'robin'})
    bt = {'left': 'neumann', 'top': 'neumann'}
    with pytest.raises(NotImplementedError):
        D.variable_density_poisson_solve(rho, f, b, dx, dy=2 * dx, boundary_types=bt)
    bad = rho.copy()
    bad[1, 0, 5] = 0.0                                                     # on the Neumann edge
    with pytest.raises(ValueError, match='positive'):
        D.variable_density_poisson_solve(bad, f, b, dx, boundary_types=bt)
    with pytest.raises(ValueError, match='same'):
        D.variable_density_poisson_solve(rho[:, :-1], f, b, dx, boundary_types=bt)
    with pytest.raises(ValueError, match='tol'):
        D.variable_density_poisson_solve(rho, f, b, dx, tol=0.0, boundary_types=bt)
    with pytest.raises(ValueError, match='top'):
        D.variable_density_poisson_solve(rho, f, {k: v for k, v in b.items() if k != 'top'}, dx, boundary_types=bt)
    with pytest.raises(ValueError, match='3 points'):
        D.variable_density_poisson_solve(rho[:, :2], f[:, :, :2], b, dx, boundary_types=bt)
    with pytest.raises(ValueError):
        D.variable_density_dataset_generator(batch_size=2, device='cpu', boundary_types={'left': 'robin'})


def test_train_refuses_neumann_boundary_types_for_the_variable_density_dataset(tmp_path):
    import json
    from poisson_cnn_amd import configs, train
    cfg = configs.hpnn_tiny()
    cfg['model']['density_input'] = True
    cfg['dataset'] = {'batch_size': 2, 'boundary_types': {'left': 'neumann'}}
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match='model does not'):
        train.main([str(path), '--dataset_type', 'variable_density', '--model', 'hpnn'])
