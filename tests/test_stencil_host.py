"""Host side of the general-stencil Jacobi smoother and of the rectangular physics-informed loss (no GPU): the per-sample coefficient rows the layer
hands to csrc/stencil.hip, the constructor's refusals, and the two guards that used to refuse what the reference accepts."""
import numpy as np
import pytest
import torch

from oracle import np_ops


def oracle_rows(dx, stencil_sizes, orders):
    """np_ops.jacobi_iterations:320-327, laid out as the kernel takes it: H taps, W taps (centres zero), 1 / diagonal."""
    coeff = np_ops.build_fd_coefficients(list(stencil_sizes), list(orders), 2)
    c = tuple(s // 2 for s in stencil_sizes)
    diag = coeff[(Ellipsis,) + c].copy()
    lu = coeff.copy()
    lu[(Ellipsis,) + c] = 0.0
    dxp = (1.0 / dx) ** np.array(orders, dtype=np.float64)
    kern = np.einsum('dij,bd->bij', lu, dxp)
    dinv = 1.0 / (dxp @ diag)
    # a cross: everything off the two centre lines is zero, so the two lines ARE the kernel
    off = kern.copy()
    off[:, c[0], :] = 0.0
    off[:, :, c[1]] = 0.0
    assert not off.any()
    return np.concatenate([kern[:, :, c[1]], kern[:, c[0], :], dinv[:, None]], axis=1)


@pytest.mark.parametrize('ss,od', [([5, 3], [2, 2]), ([7, 7], [4, 2]), ([3, 3], [2, 2])])
def test_coefficient_rows_match_the_oracle_composition(ss, od):
    """fp32 rounding: each entry is 1/dx (0.5 ulp), a power (<= 1 ulp + the amplified input error, order * 0.5 ulp), one product with an fp32-rounded
    coefficient (2 x 0.5 ulp); 1 / diagonal adds a sum and a reciprocal whose terms do not cancel (the 4th-order term outweighs the 2nd-order one
    by (1/dx)^2 >= 400).  That is at most ~6 ulp = 4e-7 relative; the bound is 1e-6 per entry."""
    from poisson_cnn_amd.layers import JacobiIterationLayer
    rng = np.random.default_rng(3)
    dx = rng.uniform(5e-3, 5e-2, (4, 2)).astype(np.float32)
    lay = JacobiIterationLayer(3, ss, od)
    rows = lay.coefficient_rows(torch.from_numpy(dx))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (4, ss[0] + ss[1] + 1) and rows.is_contiguous()
    ref = oracle_rows(dx.astype(np.float64), ss, od)
    got = rows.numpy().astype(np.float64)
    assert np.all(got[:, ss[0] // 2] == 0.0) and np.all(got[:, ss[0] + ss[1] // 2] == 0.0)
    assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref))
    assert lay.fused == (ss != [3, 3])


def test_default_layer_keeps_the_per_sweep_path():
    from poisson_cnn_amd.layers import JacobiIterationLayer
    lay = JacobiIterationLayer()
    assert lay.n == 5 and lay.stencil_sizes == [3, 3] and lay.orders == [2, 2] and lay.fused is False
    assert JacobiIterationLayer(4).n == 4                        # the models' call: L.JacobiIterationLayer(postsmoother_iterations)
    assert JacobiIterationLayer(2, fused=True).fused is True
    assert JacobiIterationLayer(2, 5, 2).stencil_sizes == [5, 5]


@pytest.mark.parametrize('ss,od', [([3, 3], [1, 2]), ([3, 3], [3, 2]), ([3, 3], [4, 2]), ([4, 3], [2, 2]), ([3, 6], [2, 2]), ([5, 5], [2, 3]),
                                   ([5, 5], [0, 2]), ([11, 3], [2, 2]), ([1, 3], [2, 2])])
def test_constructor_refuses_singular_and_impossible_stencils(ss, od):
    from poisson_cnn_amd.layers import JacobiIterationLayer
    with pytest.raises(ValueError):
        JacobiIterationLayer(3, ss, od)


def test_keras_layer_and_loss_wrapper_accept_what_the_reference_accepts():
    from poisson_cnn_amd import keras_layers as K
    from poisson_cnn_amd.losses import loss_wrapper
    lay = K.JacobiIterationLayer([5, 5], [2, 2], device='cpu')
    assert lay.layer.fused and lay.layer.n == 5
    assert K.JacobiIterationLayer(7, 4, ndims=2, n_iterations=2, device='cpu').layer.stencil_sizes == [7, 7]
    assert K.JacobiIterationLayer([3, 3], [2, 2], device='cpu').layer.fused is False
    with pytest.raises(ValueError):
        K.JacobiIterationLayer([4, 4], [2, 2], device='cpu')
    with pytest.raises(NotImplementedError):
        K.JacobiIterationLayer([3, 3], [2, 2], ndims=3, device='cpu')
    L = loss_wrapper(ndims=2, integral_loss_weight=1.0, integral_loss_config={'n_quadpts': 7}, physics_informed_loss_weight=0.5,
                     physics_informed_loss_config={'stencil_sizes': [5, 3], 'orders': 2})
    assert L.pi_stencil.shape == (2, 5, 3)
    assert np.allclose(L.pi_stencil, np_ops.build_fd_coefficients([5, 3], 2, 2))


def test_fused_launch_limits_are_exported():
    from poisson_cnn_amd import ops
    T = ops.jacobi_tile()
    assert T >= 16
    for s in (3, 5, 7, 9):
        k = ops.jacobi_k_max(s, s)
        assert k >= 1 and k == ops.jacobi_k_max(3, s) == ops.jacobi_k_max(s, 3)      # the wider axis decides
        # forward LDS: two ping-pong images and rhs, each the tile plus the k-sweep halo: within the CU's 160 KiB
        assert 3 * (T + 2 * k * (s // 2)) ** 2 * 4 <= 160 * 1024
    assert ops.jacobi_k_max(3, 3) >= 5                                              # the class default of 5 iterations is one launch
