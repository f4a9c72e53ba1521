"""The numpy twin of the diagonally scaled preconditioner (tests/varcoef_scaled_twin.py) has the properties the *_scaled entry points of
poisson_cnn_amd/csrc/varcoef.hip rest on, and the Python entry points refuse bad values before they touch a device - no GPU
needed.  33 x 47, density ratios 100 and 1000, the smooth fixture smooth_density(default_rng(0), ..); masks 0, 1 (one Neumann edge) and 15."""
import functools

import numpy as np
import pytest

from tests import varcoef_bc_twin as B
from tests import varcoef_scaled_twin as S
from tests import varcoef_twin as T

H, W = 33, 47
MASKS = [0, 1, 15]
RATIOS = [100.0, 1000.0]


@functools.lru_cache(maxsize=None)
def system(ratio, mask):
    """(A, b, sample) of the fixture; read, never written."""
    rho, f, e, dx = S.smooth_fixture(H, W, ratio)
    sample = (rho[0], f[0], {k: v[0] for k, v in e.items()}, dx[0])
    A, b = B.assemble(sample[0], sample[3], mask, sample[2], sample[1])
    return A, b, sample


@functools.lru_cache(maxsize=None)
def runs(ratio, mask):
    """(plain loop, scaled loop, trace of the scaled loop's r.z pairs), each loop (x, iterations, relative residual)."""
    A, b, (_, _, _, dx) = system(ratio, mask)
    trace = []
    return S.plain_pcg(A, b.copy(), H, W, mask, tol=1e-10), S.pcg(A, b.copy(), H, W, mask, dx, tol=1e-10, trace=trace), trace


def test_the_fixture_is_the_smooth_density_of_the_plain_twin():
    rho = S.smooth_fixture(H, W, 1000.0)[0][0]
    ref = T.smooth_density(np.random.default_rng(0), H, W, 1.0, 1000.0)
    assert np.array_equal(rho, ref.astype(np.float32).astype(np.float64)) and rho.min() == 1.0 and rho.max() == 1000.0


@pytest.mark.parametrize('mask', range(16))
def test_scaling_is_the_mean_face_coefficient_and_commutes_with_the_weights(mask):
    """d = diag(A) / diag(M) with M the constant operator of the same closure, whose diagonal is 4 / dx^2 everywhere; in the interior the mean of the
    four face coefficients; W (s M^-1 s) is symmetric, so the scaled preconditioner is self-adjoint in the W inner product."""
    h, w_, dx = 7, 9, 0.03
    rho = T.smooth_density(np.random.default_rng(3), h, w_, 1.0, 100.0)
    A, _ = B.assemble(rho, dx, mask)
    M = B.constant_operator(h, w_, mask)
    assert np.array_equal(np.diag(M), np.full(M.shape[0], 4.0))
    s = S.scaling(A, dx)
    assert np.abs(s - (A.diagonal() / (np.diag(M) / dx ** 2)) ** -0.5).max() <= 1e-14 * s.max()
    i0, i1, j0, j1 = B.unknowns(h, w_, mask)
    bi, bj = T.face_coefficients(rho)
    mean = 0.25 * (bi[:-1, 1:-1] + bi[1:, 1:-1] + bj[1:-1, :-1] + bj[1:-1, 1:])          # nodes 1..h-2 x 1..w-2
    got = (s ** -2).reshape(i1 - i0 + 1, j1 - j0 + 1)[1 - i0:h - 1 - i0, 1 - j0:w_ - 1 - j0]
    assert np.abs(got - mean).max() <= 1e-14 * mean.max()
    wts = B.weights(h, w_, mask).ravel()
    minv = S.spectral(h, w_, mask)
    P = np.stack([s * minv(s * col)[0] for col in np.eye(len(s))], axis=1)
    WP = wts[:, None] * P
    assert np.abs(WP - WP.T).max() <= 1e-12 * np.abs(WP).max()
    ev = np.linalg.eigvalsh(0.5 * (WP + WP.T))
    if mask != 15:
        assert ev.min() > 0
    else:               # one null vector, d^1/2 - positive, hence not a compatible residual: definite on sum w r = 0
        assert abs(ev[0]) <= 1e-12 * ev[-1] and ev[1] > 1e-8 * ev[-1]
        assert np.abs(P @ (1.0 / s)).max() <= 1e-12 * np.abs(P).max() * np.abs(1.0 / s).max()
        assert wts @ (1.0 / s) > 0


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('mask', MASKS)
def test_scaled_pcg_agrees_with_the_direct_solve(mask, ratio):
    A, b, (rho, f, e, dx) = system(ratio, mask)
    _, (x, it, rel), _ = runs(ratio, mask)
    direct = B.solve(rho, f, e, dx, mask)
    err = np.linalg.norm(B.embed(x, e, H, W, mask) - direct) / np.linalg.norm(direct)
    print('mask %d ratio %g: %d iterations, residual %.2e, error against spsolve %.2e' % (mask, ratio, it, rel, err))
    assert rel <= 1e-10 and err <= 1e-9
    if mask == 0:                                                        # the all-Dirichlet twin's system and direct solve are the same
        assert abs(A - T.assemble(rho, dx)).max() == 0.0
        assert np.linalg.norm(B.embed(x, e, H, W, 0) - T.solve(rho, f, e, dx)) <= 1e-9 * np.linalg.norm(direct)


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('mask', MASKS)
def test_scaled_count_is_at_most_half_the_plain_count(mask, ratio):
    (_, plain, rel_plain), (_, scaled, rel_scaled), _ = runs(ratio, mask)
    print('mask %d ratio %g: plain %d, scaled %d iterations' % (mask, ratio, plain, scaled))
    assert rel_plain <= 1e-10 and rel_scaled <= 1e-10
    assert 2 * scaled <= plain


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('mask', MASKS)
def test_rz_from_the_spectral_sum_is_the_direct_dot_product(mask, ratio):
    """sum c^2 / (lam_h + lam_w), c the coefficients of s o r, against sum w r z with z = s o M^-1 (s o r): every application of the solve."""
    trace = runs(ratio, mask)[2]
    assert len(trace) >= 10
    worst = max(abs(a - c) / abs(c) for a, c in trace)
    print('mask %d ratio %g: r.z spectral against direct, worst relative difference %.2e over %d applications' % (mask, ratio, worst, len(trace)))
    assert worst <= 1e-12


def test_constant_density_gives_the_plain_iterates():
    """rho = c: s is the constant c^1/2 and s M^-1 s = c M^-1 - a multiple of the plain preconditioner, the same iterates, converged in one."""
    _, f, e, dx = S.smooth_fixture(9, 12, 10.0)
    for mask in (0, 5, 15):
        A, b = B.assemble(np.full((9, 12), 2.5), dx[0], mask, {k: v[0] for k, v in e.items()}, f[0])
        x0, it0, _ = B.pcg(A, b.copy(), 9, 12, mask)
        x1, it1, _ = S.pcg(A, b.copy(), 9, 12, mask, dx[0])
        assert it0 == it1 == 1 and np.abs(x0 - x1).max() <= 1e-12 * np.abs(x0).max()


def test_warm_start_at_the_solution_takes_no_iteration():
    A, b, (rho, f, e, dx) = system(100.0, 1)
    i0, i1, j0, j1 = B.unknowns(H, W, 1)
    x0 = B.solve(rho, f, e, dx, 1)[i0:i1 + 1, j0:j1 + 1].ravel()
    assert S.pcg(A, b.copy(), H, W, 1, dx, x0=x0)[1] == 0


# ----------------------------------------------------------------------------- host-side argument checks of the Python entry points
def test_entry_points_refuse_unknown_values_without_a_device():
    from poisson_cnn_amd import dataset as D
    rho = np.ones((2, 9, 11), dtype=np.float32)
    f = np.zeros((2, 1, 9, 11), dtype=np.float32)
    b = {k: np.zeros((2, 11 if k in ('left', 'right') else 9), dtype=np.float32) for k in B.EDGES}
    dx = np.full((2, 1), 0.01, dtype=np.float32)
    for bad in ('jacobi', 'DST', None, ''):
        with pytest.raises(ValueError, match='preconditioner'):
            D.variable_density_poisson_solve(rho, f, b, dx, preconditioner=bad)
        with pytest.raises(ValueError, match='preconditioner'):
            D.compressible_poisson_solve(rho, f, b, dx, preconditioner=bad)
        with pytest.raises(ValueError, match='preconditioner'):
            D.variable_density_dataset_generator(batch_size=2, device='cpu', preconditioner=bad)
    with pytest.raises(ValueError, match='density_profile'):
        D.variable_density_dataset_generator(batch_size=2, device='cpu', density_profile='linear')
    # a refusal that comes later than the keyword's check shows the two values themselves are accepted
    for ok in ('dst', 'scaled'):
        with pytest.raises(ValueError, match='tol'):
            D.variable_density_poisson_solve(rho, f, b, dx, tol=0.0, preconditioner=ok, boundary_types={'left': 'neumann'})
    assert D.VARIABLE_DENSITY_PRECONDITIONERS == ('dst', 'scaled') and D.VARIABLE_DENSITY_PROFILES == ('abs', 'smooth')


def test_scaled_entry_points_are_declared_with_the_arguments_of_the_plain_ones():
    from poisson_cnn_amd import _lib
    protos = _lib.header_prototypes()
    for name in ('pcnn_varcoef_pcg_workspace', 'pcnn_varcoef_pcg_setup', 'pcnn_varcoef_pcg_iterate', 'pcnn_varcoef_bc_pcg_workspace', 'pcnn_varcoef_bc_pcg_setup',
                 'pcnn_varcoef_bc_pcg_iterate'):
        assert name + '_scaled' in protos and protos[name + '_scaled'] == protos[name], name
    assert 'pcnn_varcoef_density_smooth' in protos
