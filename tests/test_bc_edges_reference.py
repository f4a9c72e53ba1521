"""CPU: the twins of tests/bc_edges_twin.py pinned to the existing oracle before any kernel is compared with them."""
import numpy as np
import pytest
import torch

from oracle import np_ops
from tests import bc_edges_twin as T

MASKS = list(range(16))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def data(H, W, seed=0, N=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, 1, H, W)), rng.standard_normal((N, 1, H, W)), rng.uniform(5e-3, 5e-2, (N, 2))


@pytest.mark.parametrize('H,W', [(3, 3), (4, 7), (9, 6)])
def test_ring_masks_0_and_15_are_the_oracle_ring(H, W):
    x, _, _ = data(H, W)
    assert np.array_equal(T.ring(x, 0), np_ops.bc_ring(x, 'CONSTANT'))
    assert np.array_equal(T.ring(x, 15), np_ops.bc_ring(x, 'SYMMETRIC'))


@pytest.mark.parametrize('ss,od', [((3, 3), (2, 2)), ((5, 7), (4, 2)), ((9, 3), (2, 2))])
def test_sweep_with_mask_0_is_the_oracle_sweep(ss, od):
    u, rhs, dx = data(14, 13, 1)
    assert rel(T.sweeps(u, rhs, dx, 3, 0, ss, od), np_ops.jacobi_iterations(u, rhs, dx, 3, ss, od)) <= 1e-13
    # and the dtype recurrence in fp64 is the same operator, for every mask, forward and adjoint
    from tests.test_gpu_jacobi_stencil import rows_of
    r64 = rows_of(ss, od, dx, np.float64)
    for mask in (0, 15, 1, 2, 4, 8, 6):
        assert rel(T.recurrence(u, rhs, r64, ss, 2, mask, np.float64), T.sweeps(u, rhs, dx, 2, mask, ss, od)) <= 1e-13
        assert rel(T.recurrence(u, rhs, r64, ss, 2, mask, np.float64, adjoint=True), T.adjoint(u, rhs, dx, u, 2, mask, ss, od)) <= 1e-13


@pytest.mark.parametrize('mask', MASKS)
def test_3x3_sweep_is_the_ring_after_the_oracle_sweep(mask):
    """R_m J == E_m J on every point but the Dirichlet ring, which R_m leaves frozen and E_m zeroes: equal wherever the guess already satisfies its
    Dirichlet condition (the model's does: it comes out of E_m), and equal everywhere else for any guess."""
    u, rhs, dx = data(7, 9, 2)
    J = np_ops.jacobi_iterations(u, rhs, dx, 1)
    got, want = T.sweeps(u, rhs, dx, 1, mask), T.ring(J, mask)
    _, _, frozen = T.tables(7, 9, mask, 1, 1)
    assert np.array_equal(got[..., ~frozen], want[..., ~frozen]) and np.array_equal(got[..., frozen], u[..., frozen])
    u0 = T.ring(u, mask)
    assert np.array_equal(T.sweeps(u0, rhs, dx, 1, mask), T.ring(np_ops.jacobi_iterations(u0, rhs, dx, 1), mask))


@pytest.mark.parametrize('mask', MASKS)
def test_ring_adjoint_identity(mask):
    v, w, _ = data(6, 5, 3)
    lhs, rhs_ = float(np.vdot(T.ring(v, mask), w)), float(np.vdot(v, T.ring_adjoint(w, mask)))
    assert abs(lhs - rhs_) <= 1e-13 * max(abs(lhs), abs(rhs_), 1.0)
    assert not T.ring_adjoint(w, mask)[..., 0, :].any() and not T.ring_adjoint(w, mask)[..., :, -1].any()      # E_m^T w is zero on the ring


def test_corner_rule_by_hand():
    """4 x 5, left (y = 0) and top (x = 4) Neumann, right (y = 3) and bottom (x = 0) Dirichlet."""
    x = np.arange(1.0, 21.0).reshape(1, 1, 4, 5)
    #  1  2  3  4  5
    #  6  7  8  9 10
    # 11 12 13 14 15
    # 16 17 18 19 20
    want = np.array([[0., 7., 8., 9., 9.],          # (0,0): bottom is Dirichlet -> 0; (0,4): both Neumann -> the diagonal neighbour (1,3)
                     [0., 7., 8., 9., 9.],
                     [0., 12., 13., 14., 14.],
                     [0., 0., 0., 0., 0.]])         # (3,4): right is Dirichlet -> 0
    assert np.array_equal(T.ring(x, T.mask_of({'left': 'neumann', 'top': 'neumann'}))[0, 0], want)
    assert T.mask_of({'left': 'neumann', 'top': 'neumann'}) == 0b1001 and T.mask_of(None) == 0
    assert np.array_equal(T.ring(torch.tensor(x), 0b1001).numpy()[0, 0], want)
