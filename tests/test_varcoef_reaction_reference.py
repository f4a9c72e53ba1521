"""The fp64 twin of the variable-density solve with a reaction term (tests/varcoef_reaction_twin.py) against the twins that
were there before it, its own properties, and the host-side refusals of the Python entry points - no GPU."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

from tests import varcoef_bc_twin as B
from tests import varcoef_reaction_twin as R
from tests import varcoef_twin as T

MASKS = (0, 5, 10, 15)


def fixture(H, W, ratio, seed=0, c_scale=1.0):
    rng = np.random.default_rng(seed)
    rho = T.smooth_density(rng, H, W, 1.0, ratio)
    f = rng.uniform(-1, 1, (H, W))
    e = {k: rng.uniform(-1, 1, W if k in ('left', 'right') else H) for k in B.EDGES}
    dx = 0.013
    c = c_scale * T.smooth_density(rng, H, W, 0.2, 5.0) / (dx * dx)
    return rho, c, f, e, dx


@pytest.mark.parametrize('mask', MASKS)
def test_zero_reaction_gives_the_existing_systems_exactly(mask):
    rho, _, f, e, dx = fixture(12, 15, 10.0)
    AC, b = R.assemble(rho, np.zeros_like(rho), dx, mask, e, f)
    A0, b0 = B.assemble(rho, dx, mask, e, f)
    assert AC.shape == A0.shape and abs(AC - A0).max() == 0.0 and np.array_equal(b, b0)
    if mask == 0:
        assert abs(AC - T.assemble(rho, dx)).max() == 0.0 and np.array_equal(b, T.right_hand_side(rho, f, e, dx))
        # ... and with c = 0 the preconditioner is a positive multiple of the plain one: the same iterates up to rounding, the same count; both
        # stop at a relative residual of 1e-10 of a system whose preconditioned condition number is at most the density ratio 10
        x0, it0, _ = B.pcg(A0, b0.copy(), 12, 15, 0)
        x1, it1, _ = R.pcg(AC, b.copy(), rho, np.zeros_like(rho), dx, 0)
        assert it0 == it1 and np.abs(x0 - x1).max() <= 10.0 * 1e-10 * np.abs(x0).max()


@pytest.mark.parametrize('mask', MASKS)
def test_weighted_system_is_symmetric(mask):
    rho, c, _, _, dx = fixture(12, 15, 100.0)
    AC, _ = R.assemble(rho, c, dx, mask)
    WA = (sp.diags(B.weights(12, 15, mask).ravel()) @ AC).toarray()
    assert np.abs(WA - WA.T).max() <= 1e-14 * np.abs(WA).max()
    assert np.linalg.eigvalsh(0.5 * (WA + WA.T)).min() > 0.0                     # definite for every mask, 15 included


def manufactured_error(n, mask=0):
    """u = sin(pi x) sin(2 pi y) + x y, rho = 1 + x + 0.5 y, c = 3 + x on the unit square (x along rows), f from the continuous operator."""
    x, y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing='ij')
    pi = np.pi
    u = np.sin(pi * x) * np.sin(2 * pi * y) + x * y
    ux, uy = pi * np.cos(pi * x) * np.sin(2 * pi * y) + y, 2 * pi * np.sin(pi * x) * np.cos(2 * pi * y) + x
    lap = -5 * pi * pi * np.sin(pi * x) * np.sin(2 * pi * y)
    rho, c = 1 + x + 0.5 * y, 3 + x
    f = lap / rho - (ux + 0.5 * uy) / rho ** 2 - c * u
    nl, nr, nb, nt = B.flags(mask)
    e = {'left': -ux[0] if nl else u[0], 'right': ux[-1] if nr else u[-1], 'bottom': -uy[:, 0] if nb else u[:, 0], 'top': uy[:, -1] if nt else u[:, -1]}
    return np.abs(R.solve(rho, c, f, e, 1.0 / (n - 1), mask) - u).max()


def test_second_order_on_a_manufactured_solution():
    e33, e65 = manufactured_error(33), manufactured_error(65)
    print('max error 33^2 %.3e, 65^2 %.3e, factor %.3f' % (e33, e65, e33 / e65))
    assert 3.6 <= e33 / e65 <= 4.4


@pytest.mark.parametrize('mask,c_scale', [(m, s) for m in MASKS for s in (0.0, 1e-3, 1.0, 1e3) if (m, s) != (15, 0.0)])       # (15, 0) is singular: refused
def test_extreme_generalised_eigenvalues_lie_inside_the_bound(mask, c_scale):
    """v.W(A + C)v / v.W(bbar M + cbar I)v in [min(beta / bbar, c / cbar), max(..)] on a 17 x 21 problem at density ratio 100."""
    H, W = 17, 21
    rho, c, _, _, dx = fixture(H, W, 100.0, seed=3, c_scale=c_scale)
    w = B.weights(H, W, mask).ravel()
    AC, _ = R.assemble(rho, c, dx, mask)
    cbar, bbar = R.means(rho, c, mask)
    WA = w[:, None] * AC.toarray()
    WP = w[:, None] * R.preconditioner_matrix(H, W, mask, dx, cbar, bbar)
    ev = scipy.linalg.eigh(0.5 * (WA + WA.T), 0.5 * (WP + WP.T), eigvals_only=True)
    lo, hi = R.spectrum_bound(rho, c, mask)
    print('mask %d c_scale %g: eigenvalues [%.4f, %.4f] inside [%.4f, %.4f], condition %.1f <= %.1f' % (mask, c_scale, ev[0], ev[-1], lo, hi, ev[-1] / ev[0], hi / lo))
    assert lo * (1 - 1e-10) <= ev[0] and ev[-1] <= hi * (1 + 1e-10)
    # the spectral form of the preconditioner is the inverse of that matrix
    r = np.random.default_rng(1).standard_normal(AC.shape[0])
    z = R.preconditioner(H, W, mask, dx, cbar, bbar)(r)
    assert np.abs(R.preconditioner_matrix(H, W, mask, dx, cbar, bbar) @ z - r).max() <= 1e-9 * np.abs(r).max()


@pytest.mark.parametrize('mask', MASKS)
def test_twin_pcg_reaches_the_direct_solution(mask):
    H, W = 17, 21
    rho, c, f, e, dx = fixture(H, W, 100.0, seed=5)
    AC, b = R.assemble(rho, c, dx, mask, e, f)
    x, it, rel = R.pcg(AC, b.copy(), rho, c, dx, mask)
    ref = R.on_unknowns(R.solve(rho, c, f, e, dx, mask), mask).ravel()
    assert rel <= 1e-10 and it < 100 and np.abs(x - ref).max() <= 1e-8 * np.abs(ref).max()


# ----------------------------------------------------------------------------- host-side argument checks of the Python entry points
def test_entry_points_refuse_without_a_device():
    from poisson_cnn_amd import dataset as D
    N, H, W = 2, 9, 11
    rho = np.ones((N, H, W), dtype=np.float32)
    f = np.zeros((N, 1, H, W), dtype=np.float32)
    b = {k: np.zeros((N, W if k in ('left', 'right') else H), dtype=np.float32) for k in B.EDGES}
    dx = np.full((N, 1), 0.01, dtype=np.float32)
    c = np.ones((N, H, W), dtype=np.float32)
    all_neumann = {k: 'neumann' for k in B.EDGES}
    for solve in (D.variable_density_poisson_solve, D.compressible_poisson_solve):
        for bad in (-1.0, np.nan, np.inf):
            field = c.copy()
            field[1, 4, 5] = bad
            with pytest.raises(ValueError, match='reaction'):
                solve(rho, f, b, dx, reaction=field)
            with pytest.raises(ValueError, match='reaction'):
                solve(rho, f, b, dx, reaction=np.array([1.0, bad]))
        for shape in ((N, H, W + 1), (N, 2, H, W), (N + 1,), (H, W)):
            with pytest.raises(ValueError, match='reaction'):
                solve(rho, f, b, dx, reaction=np.ones(shape, dtype=np.float32))
        with pytest.raises(ValueError, match='scaled'):
            solve(rho, f, b, dx, reaction=c, preconditioner='scaled')
    zero_sample = c.copy()
    zero_sample[1] = 0.0
    with pytest.raises(ValueError, match='singular'):
        D.variable_density_poisson_solve(rho, f, b, dx, reaction=zero_sample, boundary_types=all_neumann)
    with pytest.raises(ValueError, match='singular'):
        D.variable_density_poisson_solve(rho, f, b, dx, reaction=np.array([2.0, 0.0]), boundary_types=all_neumann)
    # c is read on the unknowns only: a value on a Dirichlet node is not looked at - the refusal that comes later shows the field was accepted
    ring = c.copy()
    ring[:, 0, :] = -1.0
    for ok in (ring, c[:, None], np.array([0.0, 3.0]), np.array([[0.5], [0.0]]), 2.0):
        with pytest.raises(ValueError, match='tol'):
            D.variable_density_poisson_solve(rho, f, b, dx, reaction=ok, tol=0.0)
    with pytest.raises(ValueError, match='reaction'):
        D.variable_density_poisson_solve(rho, f, b, dx, reaction=ring, boundary_types={'left': 'neumann'})
    for bad in ((-1.0, 2.0), (3.0, 2.0), (0.0, np.inf), (1.0,)):
        with pytest.raises(ValueError, match='reaction_range'):
            D.variable_density_dataset_generator(batch_size=2, device='cpu', reaction_range=bad)
    with pytest.raises(ValueError, match='scaled'):
        D.variable_density_dataset_generator(batch_size=2, device='cpu', reaction_range=(0.0, 1.0), preconditioner='scaled')
    assert D.variable_density_dataset_generator(batch_size=2, device='cpu', reaction_range=(0.0, 1.0)).reaction_range == (0.0, 1.0)
    assert D.variable_density_dataset_generator(batch_size=2, device='cpu').reaction_range is None


def test_reaction_entry_points_are_declared_with_the_arguments_of_the_plain_ones_and_the_field():
    from poisson_cnn_amd import _lib
    protos = _lib.header_prototypes()
    for name in ('pcnn_varcoef_bc_apply', 'pcnn_varcoef_bc_pcg_setup', 'pcnn_varcoef_bc_pcg_iterate'):
        ret, args = protos[name]
        assert protos[name + '_reaction'] == (ret, args + ['const float*']), name
    assert protos['pcnn_varcoef_bc_pcg_workspace_reaction'] == protos['pcnn_varcoef_bc_pcg_workspace']
    assert protos['pcnn_varcoef_bc_pcg_finish_reaction'] == protos['pcnn_varcoef_bc_pcg_finish']
    assert protos['pcnn_varcoef_reaction_field'] == protos['pcnn_varcoef_density']
