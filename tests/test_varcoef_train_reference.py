"""The fp64 twin of the variable-density training operators (tests/varcoef_train_twin.py) against what the project already trusts: the sparse
matrix of tests/varcoef_twin.py, the oracle's 5-point sweep and residual, torch.autograd, and the sparse direct solve.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import dataset as odata
from oracle import loss as oloss
from oracle import np_ops
from tests import varcoef_train_twin as T
from tests import varcoef_twin as V

SHAPES = [(3, 3), (4, 7), (9, 12), (17, 11)]


def _fields(seed, N, H, W, lo=1.0, hi=10.0):
    rng = np.random.default_rng(seed)
    u, f = rng.standard_normal((N, H, W)), rng.standard_normal((N, H, W))
    rho = rng.uniform(lo, hi, (N, H, W))
    dx = rng.uniform(5e-3, 5e-2, N)
    return T.t64(u), T.t64(rho), T.t64(f), T.t64(dx)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize('H,W', SHAPES)
def test_operator_is_minus_the_sparse_matrix(H, W):
    """With a zero ring L u = -(A u_interior); a non-zero ring adds exactly what right_hand_side moves to b."""
    u, rho, f, dx = _fields(1, 2, H, W)
    for n in range(2):
        A = V.assemble(rho[n].numpy(), float(dx[n]))
        u0 = u[n:n + 1].clone()
        u0[:, 0, :] = u0[:, -1, :] = 0.0
        u0[:, :, 0] = u0[:, :, -1] = 0.0
        Lu = T.operator(u0, rho[n:n + 1], dx[n:n + 1])[0].numpy().ravel()
        assert _rel(Lu, -(A @ u[n, 1:-1, 1:-1].numpy().ravel())) <= 1e-12
        bc = {'left': u[n, 0, :].numpy(), 'right': u[n, -1, :].numpy(), 'bottom': u[n, :, 0].numpy(), 'top': u[n, :, -1].numpy()}
        b = V.right_hand_side(rho[n].numpy(), f[n].numpy(), bc, float(dx[n]))          # b = -f + ring terms: L u - f = b - A u_interior
        res = T.residual(u[n:n + 1], rho[n:n + 1], f[n:n + 1], dx[n:n + 1])[0].numpy().ravel()
        assert _rel(res, b - A @ u[n, 1:-1, 1:-1].numpy().ravel()) <= 1e-12


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('c', [1.0, 3.5])
def test_constant_density_is_the_five_point_problem(H, W, c):
    """rho = c: the sweep and the residual are the oracle's 5-point ones with rhs replaced by c * rhs."""
    u, _, f, dx = _fields(2, 2, H, W)
    rho = torch.full_like(u, c)
    dx2 = np.stack([dx.numpy(), dx.numpy()], 1)
    ref = np_ops.jacobi_iterations(u.numpy()[:, None], c * f.numpy()[:, None], dx2, 3)[:, 0]
    assert _rel(T.sweep(u, rho, f, dx, 3).numpy(), ref) <= 1e-12
    lap = np.stack([odata.five_point_laplacian(u[n].numpy(), float(dx[n])) for n in range(2)])
    assert _rel(c * T.residual(u, rho, f, dx).numpy(), lap - c * f.numpy()[:, 1:-1, 1:-1]) <= 1e-12
    # ... and the mean of the squared residual is the oracle's physics-informed loss
    mine = float((c * c * T.residual_loss(u, rho, f, dx)).sum()) / (2 * (H - 2) * (W - 2))
    ref = float(oloss.linear_operator_loss(c * f.numpy()[:, None], u.numpy()[:, None], dx2, [3, 3], [2, 2]))
    assert abs(mine - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize('H,W', SHAPES)
def test_hand_written_adjoints_equal_autograd(H, W):
    u, rho, f, dx = _fields(3, 3, H, W, 1.0, 100.0)
    coef = T.t64(np.random.default_rng(4).uniform(0.5, 2.0, 3))
    p = u.clone().requires_grad_(True)
    (coef * T.residual_loss(p, rho, f, dx)).sum().backward()
    assert _rel(T.residual_loss_grad(u, rho, f, dx, coef).numpy(), p.grad.numpy()) <= 1e-12
    g = T.t64(np.random.default_rng(5).standard_normal((3, H, W)))
    for n_sweeps in (1, 4):
        p = u.clone().requires_grad_(True)
        (T.sweep(p, rho, f, dx, n_sweeps) * g).sum().backward()
        assert _rel(T.sweep_adjoint(g, rho, dx, n_sweeps).numpy(), p.grad.numpy()) <= 1e-12


@pytest.mark.parametrize('H,W', [(4, 7), (9, 12), (17, 11)])
def test_sparse_solution_is_a_fixed_point_with_zero_residual(H, W):
    rng = np.random.default_rng(6)
    rho = V.smooth_density(rng, H, W, 1.0, 10.0)
    f = rng.standard_normal((H, W))
    dx = 0.02
    bc = {'left': rng.standard_normal(W), 'right': rng.standard_normal(W), 'bottom': rng.standard_normal(H), 'top': rng.standard_normal(H)}
    for a, b in (('bottom', 'left'), ('top', 'left'), ('bottom', 'right'), ('top', 'right')):      # consistent corners
        bc[a][0 if b == 'left' else -1] = bc[b][0 if a == 'bottom' else -1]
    u = T.t64(V.solve(rho, f, bc, dx)[None])
    r, ft, dxt = T.t64(rho[None]), T.t64(f[None]), T.t64([dx])
    moved = T.sweep(u, r, ft, dxt, 1)
    assert _rel(moved.numpy(), u.numpy()) <= 1e-9
    res = T.residual(u, r, ft, dxt).numpy()
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(f[1:-1, 1:-1])
