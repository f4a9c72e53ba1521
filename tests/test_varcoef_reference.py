"""The numpy / scipy twin of the variable-density Poisson solve (tests/varcoef_twin.py) has the properties the device solver rests on, and the Python
entry point refuses bad arguments before it touches a device - no GPU needed."""
import functools

import numpy as np
import pytest

from oracle import dataset as ods
from tests import varcoef_twin as T

EDGES = ('left', 'right', 'bottom', 'top')


def random_problem(seed, H, W, lo, hi, dx):
    rng = np.random.default_rng(seed)
    rho = T.smooth_density(rng, H, W, lo, hi)
    f = rng.uniform(-1, 1, (H, W))
    b = {'left': rng.uniform(-1, 1, W), 'right': rng.uniform(-1, 1, W), 'bottom': rng.uniform(-1, 1, H), 'top': rng.uniform(-1, 1, H)}
    return rho, f, b, dx


def test_matrix_is_exactly_symmetric_and_positive_definite():
    rho, _, _, dx = random_problem(1, 9, 11, 1.0, 10.0, 0.03)
    A = T.assemble(rho, dx)
    assert A.shape == (7 * 9, 7 * 9)
    assert abs(A - A.T).max() == 0.0                                   # both triangles hold the same face coefficient, not two roundings of it
    w = np.linalg.eigvalsh(A.toarray())
    assert w.min() > 0.0
    # spectral equivalence with the constant-coefficient operator: the generalised eigenvalues lie in [min beta, max beta]
    M = ods.poisson_matrix(7, 9).toarray() / dx ** 2
    g = np.linalg.eigvals(np.linalg.solve(M, A.toarray())).real
    assert 1.0 / 10.0 - 1e-12 <= g.min() and g.max() <= 1.0 + 1e-12


def test_constant_density_is_the_constant_coefficient_system():
    """rho = 2.5 everywhere: (1/2.5) lap u = f, the system of multigrid_poisson_solve with 2.5 f."""
    rng = np.random.default_rng(2)
    N, H, W = 2, 19, 23
    f = rng.uniform(-1, 1, (N, H, W))
    b = {k: rng.uniform(-1, 1, (N, W if k in ('left', 'right') else H)) for k in EDGES}
    dx = np.array([0.02, 0.045])
    ref = ods.multigrid_poisson_solve(2.5 * f, b, dx)
    got = T.solve_batch(np.full((N, H, W), 2.5), f, b, dx)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-12     # two sparse direct solves of the same fp64 system (condition ~ 1e2-1e3)
    assert np.array_equal(got[:, 0], b['left']) and np.array_equal(got[:, -1], b['right'])
    assert np.array_equal(got[:, 1:-1, 0], b['bottom'][:, 1:-1]) and np.array_equal(got[:, 1:-1, -1], b['top'][:, 1:-1])


def manufactured_error(n):
    """u = sin(pi x) sin(2 pi y) + x y, rho = 1 + x + 0.5 y on the unit square (x along axis 0), f = div((1/rho) grad u) analytically."""
    x, y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing='ij')
    u = np.sin(np.pi * x) * np.sin(2 * np.pi * y) + x * y
    rho = 1 + x + 0.5 * y
    ux = np.pi * np.cos(np.pi * x) * np.sin(2 * np.pi * y) + y
    uy = 2 * np.pi * np.sin(np.pi * x) * np.cos(2 * np.pi * y) + x
    lap = -5 * np.pi ** 2 * np.sin(np.pi * x) * np.sin(2 * np.pi * y)
    f = lap / rho - (1.0 * ux + 0.5 * uy) / rho ** 2
    b = {'left': u[0], 'right': u[-1], 'bottom': u[:, 0], 'top': u[:, -1]}
    return np.abs(T.solve(rho, f, b, 1.0 / (n - 1)) - u).max()


def test_manufactured_solution_converges_at_second_order():
    e33, e65 = manufactured_error(33), manufactured_error(65)
    factor = e33 / e65
    print('max error 33^2 %.4e, 65^2 %.4e, factor %.4f' % (e33, e65, factor))     # measured: 2.7856e-03, 6.9559e-04, 4.0046
    assert 3.5 <= factor <= 4.5


@functools.lru_cache(maxsize=None)
def pcg_count(n, ratio):
    rho, f, b, dx = random_problem(5, n, n, 1.0, ratio, 1.0 / (n - 1))
    A, rhs = T.assemble(rho, dx), T.right_hand_side(rho, f, b, dx)
    x, it, rel = T.pcg(A, rhs, (n - 2, n - 2), tol=1e-10)
    direct = T.solve(rho, f, b, dx)[1:-1, 1:-1].ravel()
    return it, rel, np.linalg.norm(x - direct) / np.linalg.norm(direct)


def test_pcg_iteration_count_does_not_depend_on_the_grid():
    """The DST preconditioner makes the condition number at most max(beta) / min(beta) = 10 at any resolution."""
    (it33, rel33, err33), (it129, rel129, err129) = pcg_count(33, 10.0), pcg_count(129, 10.0)
    print('iterations at 33^2: %d, at 129^2: %d' % (it33, it129))                  # measured: 33 and 33
    assert abs(it33 - it129) <= 1
    assert rel33 <= 1e-10 and rel129 <= 1e-10
    assert err33 < 1e-8 and err129 < 1e-8          # error <= cond(M^-1 A) * relative residual in the matching norms; two digits of slack for the 2-norm
    # sqrt(kappa) estimate: the error bound 2 ((sqrt(k) - 1) / (sqrt(k) + 1))^i reaches 1e-10 after 37 iterations at kappa = 10
    bound = int(np.ceil(np.log(2e10) / -np.log((np.sqrt(10.0) - 1) / (np.sqrt(10.0) + 1))))
    assert it33 <= bound + 8


def test_exact_preconditioner_converges_in_one_iteration():
    rho, f, b, dx = random_problem(6, 21, 26, 1.0, 1.0, 0.04)
    _, it, rel = T.pcg(T.assemble(rho, dx), T.right_hand_side(rho, f, b, dx), (19, 24))
    assert it == 1 and rel < 1e-12


# ----------------------------------------------------------------------------- host-side argument checks of the Python entry point
def solve_args(N=2, H=9, W=11):
    rho = np.ones((N, H, W), dtype=np.float32)
    f = np.zeros((N, 1, H, W), dtype=np.float32)
    b = {k: np.zeros((N, W if k in ('left', 'right') else H), dtype=np.float32) for k in EDGES}
    return rho, f, b, np.full((N, 1), 0.01, dtype=np.float32)


def test_entry_point_refuses_bad_arguments_without_a_device():
    from poisson_cnn_amd import dataset as D
    rho, f, b, dx = solve_args()
    with pytest.raises(NotImplementedError):
        D.variable_density_poisson_solve(rho, f, b, dx, dy=2 * dx)
    with pytest.raises(NotImplementedError):
        D.variable_density_poisson_solve(rho, f, b, np.stack([dx[:, 0], 2 * dx[:, 0]], 1))
    with pytest.raises(NotImplementedError):
        D.compressible_poisson_solve(rho, f, b, 0.01, 0.02)
    bad = rho.copy()
    bad[1, 4, 5] = 0.0
    with pytest.raises(ValueError, match='positive'):
        D.variable_density_poisson_solve(bad, f, b, dx)
    bad[1, 4, 5] = -1.0
    with pytest.raises(ValueError, match='positive'):
        D.variable_density_poisson_solve(bad, f, b, dx, dy=dx)            # an equal dy passes the spacing check
    with pytest.raises(ValueError, match='same'):
        D.variable_density_poisson_solve(rho[:, :-1], f, b, dx)
    with pytest.raises(ValueError, match='tol'):
        D.variable_density_poisson_solve(rho, f, b, dx, tol=0.0)
    with pytest.raises(ValueError, match='max_iterations'):
        D.variable_density_poisson_solve(rho, f, b, dx, max_iterations=0)
    with pytest.raises(ValueError, match='check_every'):
        D.variable_density_poisson_solve(rho, f, b, dx, check_every=0)
    with pytest.raises(ValueError, match='top'):
        D.variable_density_poisson_solve(rho, f, {k: v for k, v in b.items() if k != 'top'}, dx)
    with pytest.raises(ValueError, match='initial_guesses'):
        D.variable_density_poisson_solve(rho, f, b, dx, initial_guesses=np.zeros((2, 9, 12)))
    with pytest.raises(ValueError, match='3 points'):
        D.variable_density_poisson_solve(rho[:, :2], f[:, :, :2], b, dx)


def test_generator_refuses_bad_ranges_without_a_device():
    from poisson_cnn_amd import dataset as D
    for kw in ({'density_range': (0.0, 1.0)}, {'density_range': (2.0, 1.0)}, {'boundaries': 'periodic'}, {'rhs_smoothness_range': (1, 4)}):
        with pytest.raises(ValueError):
            D.variable_density_dataset_generator(batch_size=2, device='cpu', **kw)
