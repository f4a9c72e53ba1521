"""Pins tests/varcoef_jacobi_grad_twin.py, the float64 reference of the smoother's gradients w.r.t. u, rho and rhs: its two
routes - torch.autograd through the sweep written with plain torch ops, and the closed forms the kernel implements - agree to 1e-9 rel-L2, and its
sweep is the sweep of the existing smoother twin (tests/varcoef_train_bc_twin.py, assembled node by node from the definition)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import varcoef_jacobi_grad_twin as J
from tests import varcoef_train_bc_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 3), (4, 5), (9, 12)]
MASKS = [0, 1, 2, 4, 8, 6, 9, 15]
SWEEPS = [1, 2, 5]
TOL = 1e-9


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('n_sweeps', SWEEPS)
def test_closed_forms_equal_autograd_through_the_sweep(shape, n_sweeps):
    H, W = shape
    u, rho, rhs, gbar, dx = J.case(H, W)                  # the 100 : 1 jump along the diagonal, a dx per sample
    assert len(set(dx.tolist())) == len(dx) and rho.max() / rho.min() > 50.0
    for mask in MASKS:
        for n in range(u.shape[0]):
            _, auto = J.autograd_grads(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, gbar[n])
            hand = J.closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, gbar[n])
            for k in J.KEYS:
                assert float(auto[k].abs().max()) > 0.0, (mask, k)
                assert J.rel_l2(hand[k], auto[k]) <= TOL, (mask, n, k, J.rel_l2(hand[k], auto[k]))
            # rhs is read on the unknowns only; a frozen node passes its gradient straight through when no unknown reads it
            assert not bool(hand['rhs'][~J.unknown_mask(H, W, mask)].any())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_sweep_is_the_smoother_twins_sweep(shape):
    H, W = shape
    u, rho, rhs, _, dx = J.case(H, W)
    for mask in MASKS:
        for n_sweeps in SWEEPS:
            for n in range(u.shape[0]):
                mine = J.sweep(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps)[-1].numpy()
                theirs = T.sweep(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps)
                assert T.rel_l2(mine, theirs) <= 1e-12, (mask, n_sweeps, n)
                # the Dirichlet nodes are frozen
                frozen = ~J.unknown_mask(H, W, mask).numpy()
                assert np.array_equal(mine[frozen], u[n][frozen])


@pytest.mark.parametrize('mask', [0, 9, 15])
def test_chain_into_the_residual(mask):
    """smooth -> residual loss: the twin's residual is the existing loss twin's, and the gradients formed the way the tape forms them equal autograd
    through the whole chain."""
    H, W, n_sweeps = 9, 12, 2
    u, rho, rhs, _, dx = J.case(H, W)
    for n in range(u.shape[0]):
        coef = 0.7 * dx[n] ** 4
        mine = float(J.residual_loss(J._t(u[n]), J._t(rho[n]), J._t(rhs[n]), dx[n], mask, coef))
        assert abs(mine - coef * T.loss(u[n], rho[n], rhs[n], dx[n], mask)) <= 1e-12 * abs(mine)
        auto = J.chain_autograd(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, coef)
        hand = J.chain_closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, coef)
        for k in J.KEYS:
            assert J.rel_l2(hand[k], auto[k]) <= TOL, (n, k, J.rel_l2(hand[k], auto[k]))


def test_float32_closed_form_is_a_floor_not_the_reference():
    """`reference` hands the GPU suite the float64 gradients and the error of the same formulas in float32: small, and not zero."""
    ref, floor = J.reference(9, 12, 9, 5)
    for k in J.KEYS:
        assert ref[k].dtype == torch.float64 and 0.0 < floor[k] < 1e-4, (k, floor[k])


def test_header_declares_the_entry_point_and_the_library_binds_it():
    """The C ABI of the feature, as tests/test_host_logic.py checks every entry point: exported, and bound with the argtypes parsed from the header."""
    from poisson_cnn_amd import _lib
    protos = _lib.header_prototypes()
    ptr, cptr = 'float*', 'const float*'
    assert protos['pcnn_varcoef_bc_jacobi_bwd_inputs'] == ('int', ['pcnn_handle', 'int', 'int', 'int', 'int', cptr, cptr, cptr, cptr, cptr, 'int', ptr, ptr, ptr])
    assert protos['pcnn_varcoef_jacobi_bwd_inputs_workspace'] == ('size_t', ['int', 'int', 'int', 'int'])
    raw = ctypes.CDLL(os.path.join(ROOT, 'poisson_cnn_amd', 'libpcnn.so'))
    assert hasattr(raw, 'pcnn_varcoef_bc_jacobi_bwd_inputs') and hasattr(raw, 'pcnn_varcoef_jacobi_bwd_inputs_workspace')
    lib = _lib.load()
    fn = lib.pcnn_varcoef_bc_jacobi_bwd_inputs
    assert fn.argtypes is not None and len(fn.argtypes) == 14 and fn.restype is ctypes.c_int
    # the workspace query needs no GPU: n iterates and two gradient fields of N H W floats; 0 for what the call refuses
    ws = lib.pcnn_varcoef_jacobi_bwd_inputs_workspace
    assert ws(3, 17, 65, 5) == ws(ctypes.c_int(3), 17, 65, 5) == (5 + 2) * 3 * 17 * 65 * 4
    assert ws(8, 1024, 1024, 100) == 102 * 8 * 1024 * 1024 * 4          # beyond 32 bits
    assert ws(3, 2, 65, 5) == 0 and ws(3, 17, 65, 0) == 0
    with pytest.raises(ctypes.ArgumentError):
        ws(3, 17, 65, 2.5)
