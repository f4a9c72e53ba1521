"""Pins tests/varcoef_grad_twin.py (CPU, float64): its dense operator against tests/varcoef_bc_twin.assemble, and the closed-form gather formulas
the kernels of csrc/varcoef_grad.hip implement against torch.autograd through the dense solve / the dense residual."""
import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_grad_twin as G

SHAPES = [(5, 4), (7, 9)]
SOLVE_MASKS = [0, 1, 6, 9]
KEYS = ('rho', 'rhs') + B.EDGES


def _sample(H, W, seed):
    """rho in [1, 100] with a jump, f and nonzero data on every edge, dx, weights of the objective."""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(1.0, 10.0, (H, W))
    rho[H // 2:, : W // 2 + 1] = rng.uniform(50.0, 100.0, (H - H // 2, W // 2 + 1))
    f = rng.standard_normal((H, W))
    edges = {k: rng.standard_normal(W if k in ('left', 'right') else H) + 0.25 for k in B.EDGES}
    return rho, f, edges, float(rng.uniform(0.05, 0.2)), rng.standard_normal((H, W))


@pytest.mark.parametrize('mask', SOLVE_MASKS + [15])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_operator_is_that_of_the_solver_twin(shape, mask):
    H, W = shape
    rho, f, edges, dx, _ = _sample(H, W, 10 * H + mask)
    A, b = G.assemble(rho, dx, mask, edges, f)
    A0, b0 = B.assemble(rho, dx, mask, edges, f)
    A0 = A0.toarray()
    assert np.abs(A.numpy() - A0).max() <= 1e-13 * np.abs(A0).max()
    assert np.abs(b.numpy() - b0).max() <= 1e-13 * np.abs(b0).max()


@pytest.mark.parametrize('mask', SOLVE_MASKS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_closed_form_gradients_equal_autograd_through_the_dense_solve(shape, mask):
    H, W = shape
    rho, f, edges, dx, ubar = _sample(H, W, 100 * H + mask)
    u, auto = G.solve_grads(rho, f, edges, dx, mask, ubar)
    assert np.abs(u.numpy() - B.solve(rho, f, edges, dx, mask)).max() <= 1e-10 * np.abs(u.numpy()).max()
    lam = G.adjoint(rho, dx, mask, ubar)
    assert not bool(lam[~G.unknown_mask(H, W, mask)].any())
    hand = G.closed_form(lam, u, rho, dx, mask, edges, ubar)
    for k in KEYS:
        assert float(auto[k].abs().max()) > 0, k
        assert G.rel_l2(hand[k], auto[k]) <= 1e-9, (k, G.rel_l2(hand[k], auto[k]))


@pytest.mark.parametrize('mask', SOLVE_MASKS + [15])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_closed_form_loss_gradients_equal_autograd(shape, mask):
    H, W = shape
    rho, f, _, dx, pred = _sample(H, W, 1000 * H + mask)
    loss, auto = G.loss_grads(pred, rho, f, dx, mask, 0.75)
    hand_loss, hand = G.loss_closed_form(pred, rho, f, dx, mask, 0.75)
    assert abs(float(hand_loss) - float(loss)) <= 1e-12 * float(loss)
    for k in ('rhs', 'rho'):
        assert G.rel_l2(hand[k], auto[k]) <= 1e-9, (k, G.rel_l2(hand[k], auto[k]))
    # rhs is read on the unknowns only, rho on every node that touches one
    assert not bool(hand['rhs'][~G.unknown_mask(H, W, mask)].any())


@pytest.mark.parametrize('mask', [0, 1, 6, 9, 4, 8])
def test_overwritten_dirichlet_corner_entries_get_no_gradient(mask):
    H, W = 5, 4
    rho, f, edges, dx, ubar = _sample(H, W, 7 + mask)
    u, auto = G.solve_grads(rho, f, edges, dx, mask, ubar)
    hand = G.closed_form(G.adjoint(rho, dx, mask, ubar), u, rho, dx, mask, edges, ubar)
    nl, nr, nb, nt = B.flags(mask)
    checked = 0
    for k, dirichlet in (('bottom', not nb), ('top', not nt)):
        for idx, row_dirichlet in ((0, not nl), (-1, not nr)):
            if dirichlet and row_dirichlet:                         # the row's array owns the corner; the column's entry is overwritten
                assert float(auto[k][idx]) == 0.0 and float(hand[k][idx]) == 0.0, (k, idx)
                row = 'left' if idx == 0 else 'right'
                col = 0 if k == 'bottom' else -1
                assert float(hand[row][col]) == float(ubar[idx, col])        # a Dirichlet corner touches no unknown: the direct term alone
                checked += 1
    assert checked == sum(1 for c in ((nl, nb), (nl, nt), (nr, nb), (nr, nt)) if not c[0] and not c[1])


def test_committed_descent_step_makes_the_twin_objective_fall_monotonically():
    """The density-identification problem of tests/test_gpu_varcoef_grad.py on the twin: GD_STEP is small enough for plain gradient descent."""
    hist = G.gd_run(G.GD_STEP)
    assert len(hist) == G.GD_STEPS + 1 and all(b < a for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] < 0.25 * hist[0]
