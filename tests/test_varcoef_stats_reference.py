"""The twin of pcnn_varcoef_error_stats (tests/error_stats_twin.py with rho) pinned against the twins that were there before it - no GPU."""
import numpy as np
import pytest

from tests import error_stats_twin as ES, varcoef_twin as VT

N, H, W = 2, 9, 12


def _fields(seed=3, zero_edges=False):
    rng = np.random.default_rng(seed)
    pred, target, rhs = rng.standard_normal((N, H, W)), rng.standard_normal((N, H, W)), rng.standard_normal((N, H, W)) * 30
    rho = rng.uniform(1.0, 10.0, (N, H, W))
    dx = rng.uniform(5e-3, 5e-2, N)
    if zero_edges:
        pred[:, 0] = pred[:, -1] = 0.0
        pred[:, :, 0] = pred[:, :, -1] = 0.0
    return pred, target, rho, rhs, dx


def test_zero_edges_give_the_residual_of_the_assembled_system():
    """sum r^2 = ||b - A u||^2 and sum f^2 = ||b||^2 with the matrix and right-hand side of tests/varcoef_twin.py, to 1e-12."""
    pred, target, rho, rhs, dx = _fields(zero_edges=True)
    got = ES.error_stats(pred, target, rhs, dx, rho)
    zero = {'left': np.zeros(W), 'right': np.zeros(W), 'bottom': np.zeros(H), 'top': np.zeros(H)}
    for n in range(N):
        b = VT.right_hand_side(rho[n], rhs[n], zero, dx[n])
        res = b - VT.assemble(rho[n], dx[n]) @ pred[n, 1:-1, 1:-1].ravel()
        assert abs(got[n, 5] - res @ res) <= 1e-12 * (res @ res)
        assert abs(got[n, 6] - np.abs(res).max()) <= 1e-12 * np.abs(res).max()
        assert abs(got[n, 7] - b @ b) <= 1e-12 * (b @ b)


def test_nonzero_edges_enter_as_dirichlet_neighbours():
    """With edge values the residual is that of the system whose right-hand side holds them - and sum f^2 is then NOT ||b||^2."""
    pred, _, rho, rhs, dx = _fields(seed=4)
    got = ES.error_stats(pred, None, rhs, dx, rho)
    for n in range(N):
        edges = {'left': pred[n, 0], 'right': pred[n, -1], 'bottom': pred[n, :, 0], 'top': pred[n, :, -1]}
        b = VT.right_hand_side(rho[n], rhs[n], edges, dx[n])
        res = b - VT.assemble(rho[n], dx[n]) @ pred[n, 1:-1, 1:-1].ravel()
        assert abs(got[n, 5] - res @ res) <= 1e-12 * (res @ res)
        assert abs(got[n, 7] - b @ b) > 1e-3 * (b @ b)


def test_constant_density_is_the_constant_coefficient_residual():
    """rho = c: r = (lap pred - c f) / c, the residual tests/error_stats_twin.py computes for the right-hand side c f, scaled by 1 / c."""
    pred, target, _, rhs, dx = _fields(seed=5)
    c = 2.5
    got = ES.error_stats(pred, target, rhs, dx, np.full((N, H, W), c))
    ref = ES.error_stats(pred, target, c * rhs, np.stack([dx, dx], 1))
    assert np.allclose(got[:, :5], ref[:, :5], rtol=1e-14, atol=0)
    assert np.allclose(got[:, 5], ref[:, 5] / c ** 2, rtol=1e-12, atol=0)
    assert np.allclose(got[:, 6], ref[:, 6] / c, rtol=1e-12, atol=0)
    assert np.allclose(got[:, 7], ref[:, 7] / c ** 2, rtol=1e-12, atol=0)


def test_float32_terms_are_float32_and_close_to_the_float64_ones():
    pred, target, rho, rhs, dx = (a.astype(np.float32) for a in _fields(seed=6))
    r32, r64 = ES.residual(pred, rho, rhs, dx, np.float32), ES.residual(pred, rho, rhs, dx, np.float64)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == (N, H - 2, W - 2)
    assert 0 < np.abs(r32 - r64).max() <= 1e-5 * np.abs(r64).max()
    a, b = ES.error_stats(pred, target, rhs, dx, rho, float32_terms=True), ES.error_stats(pred, target, rhs, dx, rho)
    assert np.array_equal(a[:, [2, 4, 7]], b[:, [2, 4, 7]])               # |e| and |t| maxima and f are exact in either mode
    assert np.allclose(a, b, rtol=1e-5, atol=0) and not np.array_equal(a[:, 5], b[:, 5])
    # one interior point by hand, in the documented order
    p, d, f = pred[0, :3, :3], rho[0, :3, :3], rhs[0, 1, 1]
    two = np.float32(2)
    t = [(two / (d[1, 1] + d[i, j])) * (p[i, j] - p[1, 1]) for i, j in ((0, 1), (2, 1), (1, 0), (1, 2))]
    want = ((t[0] + t[1]) + (t[2] + t[3])) * (np.float32(1) / (dx[0] * dx[0])) - f
    assert want.dtype == np.float32 and want == r32[0, 0, 0]


def test_null_fields_layouts_and_refusals():
    pred, target, rho, rhs, dx = _fields(seed=7)
    full = ES.error_stats(pred, target, rhs, dx, rho)
    no_t, no_f = ES.error_stats(pred, None, rhs, dx, rho), ES.error_stats(pred, target)
    assert np.all(no_t[:, :5] == 0) and np.array_equal(no_t[:, 5:], full[:, 5:])
    assert np.all(no_f[:, 5:] == 0) and np.array_equal(no_f[:, :5], full[:, :5])
    assert np.array_equal(ES.error_stats(pred[:, None], target[:, None], rhs[:, None], dx[:, None], rho[:, None]), full)
    assert np.array_equal(ES.error_stats(pred[..., None], target, rhs, dx, rho), full)
    with pytest.raises(ValueError):
        ES.error_stats(pred, target, rhs, dx, None)
    with pytest.raises(ValueError):
        ES.error_stats(pred, target, rhs, rho=rho)
    with pytest.raises(ValueError):
        ES.error_stats(pred[:, :2], target[:, :2], rhs[:, :2], dx, rho[:, :2])
