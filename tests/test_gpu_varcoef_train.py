"""The fp32 kernels of csrc/varcoef_train.hip - flux-form residual loss and its gradient, the variable-density Jacobi sweeps and their adjoint -
against the fp64 twin of tests/varcoef_train_twin.py (pinned to the oracle by tests/test_varcoef_train_reference.py).

Shapes: the smallest that meet every edge of the tilings.  The loss kernels own 16 x 64 tiles (of interior nodes forward, of all nodes backward),
the sweeps 64 x 64 tiles of nodes.  Data: random fields of unit scale (no cancellation), rho in pcnn_varcoef_density's range (1, 10).
Bounds (the project's own): rel-L2 <= 2e-6 for dpred, the sweeps and their adjoints, 2e-5 relative for the per-sample loss sums."""
import functools

import numpy as np
import pytest
import torch

from tests import varcoef_train_twin as T

pytestmark = pytest.mark.gpu

FIELD_TOL, SUM_TOL = 2e-6, 2e-5
SHAPES = [
    (1, 3, 3),          # one interior node
    (2, 4, 7),
    (2, 19, 67),        # H-2, W-2 one more than the 16 x 64 tile
    (2, 17, 65),        # ... one less (and H, W one more than the backward's node tile)
    (1, 67, 67),        # H-2, W-2 one more than the sweeps' 64 x 64 tile
    (1, 65, 65),        # ... one less (and H, W one more)
    (3, 33, 130),       # three spacings and density ratios 1, 10, 100 in one batch
]
IDS = ['%dx%dx%d' % s for s in SHAPES]


@pytest.fixture(scope='module')
def ops():
    from poisson_cnn_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(N, H, W):
    """fp32-rounded host fields (read-only) as float64 tensors: u, rho, rhs, g (N,H,W), dx (N,), coef (N,)."""
    rng = np.random.default_rng(1000 * H + W)
    f32 = lambda a: T.t64(np.asarray(a, dtype=np.float32))
    u, rhs, g = (f32(rng.standard_normal((N, H, W))) for _ in range(3))
    if (N, H, W) == (3, 33, 130):
        rho = f32(np.stack([np.ones((H, W)), rng.uniform(1.0, 10.0, (H, W)), rng.uniform(1.0, 100.0, (H, W))]))
        rho[1, 0, 0], rho[1, 1, 1], rho[2, 0, 0], rho[2, 1, 1] = 1.0, 10.0, 1.0, 100.0        # the ratios are met exactly
        dx = f32([0.005, 0.02, 0.05])
    else:
        rho = f32(rng.uniform(1.0, 10.0, (N, H, W)))
        dx = f32(rng.uniform(5e-3, 5e-2, N))
    coef = f32(rng.uniform(0.5, 2.0, N) * float(dx.min()) ** 4)           # the gradient's scale is 1 / dx^4: keeps dpred of unit order
    return u, rho, rhs, g, dx, coef


def _dev(*ts):
    return [t.to(device='cuda', dtype=torch.float32).contiguous() for t in ts]


def _sweep_counts(ops):
    k = ops.varcoef_jacobi_k_max()
    return [1, k, k + 1, 2 * k + 1]


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pi_loss_partials(ops, shape):
    u, rho, rhs, _, dx, _ = _case(*shape)
    du, drho, drhs, ddx = _dev(u, rho, rhs, dx)
    got = ops.varcoef_pi_loss_partials(du, drho, drhs, ddx).cpu().double()
    ref = T.residual_loss(u, rho, rhs, dx)
    rel = ((got - ref).abs() / ref).max().item()
    print('pi_loss_partials %s: max relative error %.3g' % (shape, rel))
    assert rel <= SUM_TOL


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pi_loss_bwd(ops, shape):
    u, rho, rhs, g, dx, coef = _case(*shape)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)
    got = ops.varcoef_pi_loss_bwd(du, drho, drhs, ddx, dcoef, torch.zeros_like(du))
    rel = T.rel_l2(got, T.residual_loss_grad(u, rho, rhs, dx, coef))
    print('pi_loss_bwd %s: rel-L2 %.3g' % (shape, rel))
    assert rel <= FIELD_TOL
    # it adds into what dpred holds: one fp32 addition per node on top of the same product
    acc = ops.varcoef_pi_loss_bwd(du, drho, drhs, ddx, dcoef, dg.clone())
    assert torch.equal(acc, dg + got)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_jacobi_forward_and_adjoint(ops, shape):
    u, rho, rhs, g, dx, _ = _case(*shape)
    du, drho, drhs, dg, ddx = _dev(u, rho, rhs, g, dx)
    zero = torch.zeros_like(u)
    for n in _sweep_counts(ops):
        out = ops.varcoef_jacobi(du, drho, drhs, ddx, n)
        rel = T.rel_l2(out, T.sweep(u, rho, rhs, dx, n))
        adj = ops.varcoef_jacobi_bwd(dg, drho, ddx, n)
        rel_adj = T.rel_l2(adj, T.sweep_adjoint(g, rho, dx, n))
        print('jacobi %s, %d sweeps: forward rel-L2 %.3g, adjoint %.3g' % (shape, n, rel, rel_adj))
        assert rel <= FIELD_TOL and rel_adj <= FIELD_TOL
        # the ring stays frozen, bit for bit
        ring = torch.ones(shape[1:], dtype=torch.bool, device='cuda')
        ring[1:-1, 1:-1] = False
        assert torch.equal(out[:, ring], du[:, ring])
        # <J^T g, v> = <g, J v - J 0>: both sides from the kernels, summed in fp64
        lin = out.double() - ops.varcoef_jacobi(_dev(zero)[0], drho, drhs, ddx, n).double()
        lhs, rhs_ = float((adj.double() * du.double()).sum()), float((dg.double() * lin).sum())
        print('    adjoint identity: |lhs - rhs| / |rhs| = %.3g' % (abs(lhs - rhs_) / abs(rhs_)))
        assert abs(lhs - rhs_) <= 1e-5 * abs(rhs_)


def test_unit_density_is_the_constant_coefficient_kernels(ops):
    """rho = 1: the sweeps are ops.jacobi_fused with the 5-point coefficients, the loss sums ops.pi_loss_partials with the 3 x 3 stencil."""
    from poisson_cnn_amd.layers import JacobiIterationLayer
    u, _, rhs, g, dx, _ = _case(3, 33, 130)
    du, drhs, dg, ddx = _dev(u, rhs, g, dx)
    one = torch.ones_like(du)
    dx2 = torch.stack([ddx, ddx], 1).contiguous()
    for n in _sweep_counts(ops):
        lay = JacobiIterationLayer(n, fused=True)
        ref = lay.forward(du.unsqueeze(-1), drhs.unsqueeze(-1), dx2).squeeze(-1)
        rel = T.rel_l2(ops.varcoef_jacobi(du, one, drhs, ddx, n), ref)
        rel_adj = T.rel_l2(ops.varcoef_jacobi_bwd(dg, one, ddx, n), lay.backward(dg.unsqueeze(-1)).squeeze(-1))
        print('rho = 1, %d sweeps: forward vs jacobi_fused %.3g, adjoint %.3g' % (n, rel, rel_adj))
        assert rel <= FIELD_TOL and rel_adj <= FIELD_TOL
    lap = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], device='cuda')
    kern = (lap[None] / ddx[:, None, None] ** 2).contiguous()
    ref = ops.pi_loss_partials(du, drhs, kern).double()
    got = ops.varcoef_pi_loss_partials(du, one, drhs, ddx).double()
    rel = ((got - ref).abs() / ref).max().item()
    print('rho = 1: loss sums vs pi_loss_partials %.3g' % rel)
    assert rel <= SUM_TOL
    coef = torch.full((3,), 1e-8, device='cuda')
    rel = T.rel_l2(ops.varcoef_pi_loss_bwd(du, one, drhs, ddx, coef, torch.zeros_like(du)), ops.pi_loss_bwd(du, drhs, kern, coef, torch.zeros_like(du)))
    print('rho = 1: dpred vs pi_loss_bwd %.3g' % rel)
    assert rel <= FIELD_TOL


def test_two_runs_are_bit_equal_and_a_sample_does_not_see_its_batch(ops):
    u, rho, rhs, g, dx, coef = _case(3, 33, 130)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)
    n = ops.varcoef_jacobi_k_max() + 1

    def run(s):
        a = [t[s].contiguous() for t in (du, drho, drhs, dg, ddx, dcoef)]
        return (ops.varcoef_pi_loss_partials(a[0], a[1], a[2], a[4]), ops.varcoef_pi_loss_bwd(a[0], a[1], a[2], a[4], a[5], torch.zeros_like(a[0])),
                ops.varcoef_jacobi(a[0], a[1], a[2], a[4], n), ops.varcoef_jacobi_bwd(a[3], a[1], a[4], n))
    first, second = run(slice(0, 3)), run(slice(0, 3))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    alone = run(slice(1, 2))
    for a, b in zip(first, alone):
        assert torch.equal(a[1:2], b)


def test_argument_checks(ops):
    u, rho, rhs, g, dx, coef = _case(2, 4, 7)
    du, drho, drhs, ddx = _dev(u, rho, rhs, dx)
    with pytest.raises(ValueError, match='contiguous'):
        ops.varcoef_jacobi(du.transpose(1, 2), drho.transpose(1, 2), drhs.transpose(1, 2), ddx, 1)
    with pytest.raises(ValueError, match='points'):
        ops.varcoef_jacobi(du, drho[:, :3].contiguous(), drhs, ddx, 1)
    with pytest.raises(ValueError, match='n_sweeps'):
        ops.varcoef_jacobi(du, drho, drhs, ddx, 0)
    with pytest.raises(ValueError, match='3 points'):
        ops.varcoef_pi_loss_partials(du[:, :2].contiguous(), drho[:, :2].contiguous(), drhs[:, :2].contiguous(), ddx)
    with pytest.raises(ValueError, match='dx'):
        ops.varcoef_pi_loss_partials(du, drho, drhs, ddx[:1])


def test_solver_solution_is_a_fixed_point_of_the_sweeps(ops):
    """variable_density_poisson_solve's solution under k_max sweeps: fp32 rounding on an fp32-rounded fixed point.  Measured on an MI355X: see the
    table of DESIGN.md section 17."""
    from poisson_cnn_amd import dataset as D
    gen = D.variable_density_dataset_generator(batch_size=2, output_shape=(33, 47), seed=3)
    (stack, dx), soln = gen[0]
    rhs, rho = stack[:, 0].contiguous(), stack[:, 1].contiguous()
    u = soln[:, 0].contiguous()
    moved = ops.varcoef_jacobi(u, rho, rhs, dx.reshape(-1).contiguous(), ops.varcoef_jacobi_k_max())
    rel = T.rel_l2(moved, u)
    print('solver solution under %d sweeps moves by rel-L2 %.3g' % (ops.varcoef_jacobi_k_max(), rel))
    assert rel <= 1e-5                       # measured on an MI355X: 9.2e-8
