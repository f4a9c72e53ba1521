"""The fp32 kernels of csrc/varcoef_train.hip with per-edge Neumann boundaries (the pcnn_varcoef_bc_* entry points) against the
fp64 twin of tests/varcoef_train_bc_twin.py (pinned by tests/test_varcoef_train_bc_reference.py) on the same fp32-rounded inputs.

Data: random fields of unit scale, rho in (1, 10) - the last sample of the 19 x 70 and 66 x 130 batches in (1, 100) with the ratio met exactly -, one
spacing per sample, N = 3.  Shapes: the loss kernels own 16 x 64 tiles of unknowns (forward) and of nodes (backward): 3 x 3 (every node an unknown at
mask 15, Neumann/Neumann corners), 3 x 4, 18 x 66 (exactly one interior tile: a Neumann edge adds a second tile row or column) and 19 x 70; the
sweeps own 64 x 64 tiles of nodes: 65 x 67 (a last tile one row thin) and 66 x 130.  Bounds: those of the all-Dirichlet kernels
(tests/test_gpu_varcoef_train.py): 2e-5 relative for the loss sums, rel-L2 2e-6 for dpred, the sweeps and their adjoints, 1e-5
of the inner product for the adjoint identity.  Run with -s for the measured maxima (DESIGN.md section 20 holds a copy)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_train_bc_twin as BT

pytestmark = pytest.mark.gpu

FIELD_TOL, SUM_TOL, DOT_TOL = 2e-6, 2e-5, 1e-5
N = 3
LOSS_SHAPES = [(3, 3), (3, 4), (18, 66), (19, 70)]
SWEEP_SHAPES = [(65, 67), (66, 130)]
ALL_MASKS = list(range(16))
SWEEP_MASKS = [0, 1, 2, 4, 8, 3, 12, 5, 11, 15]
SWEEP_COUNTS = [1, 8, 9, 17]          # one launch, the launch maximum, chains of two and of three


@pytest.fixture(scope='module')
def ops():
    from poisson_cnn_amd import ops
    assert ops.varcoef_jacobi_k_max() == 8          # what SWEEP_COUNTS is built around
    return ops


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """fp32-rounded host fields (read-only), float64: u, rho, rhs, g (N,H,W), dx (N,), coef (N,)."""
    rng = np.random.default_rng(2000 * H + W)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    u, rhs, g = (f32(rng.standard_normal((N, H, W))) for _ in range(3))
    rho = rng.uniform(1.0, 10.0, (N, H, W))
    if (H, W) in ((19, 70), (66, 130)):
        rho[2] = rng.uniform(1.0, 100.0, (H, W))
        rho[2, 0, 0], rho[2, 1, 1] = 1.0, 100.0
    rho = f32(rho)
    dx = f32(rng.uniform(5e-3, 5e-2, N))
    coef = f32(rng.uniform(0.5, 2.0, N) * float(dx.min()) ** 4)       # the gradient's scale is 1 / dx^4: keeps dpred of unit order
    for a in (u, rho, rhs, g, dx, coef):
        a.setflags(write=False)
    return u, rho, rhs, g, dx, coef


def _dev(*arrays):
    return [torch.tensor(a, device='cuda', dtype=torch.float32).contiguous() for a in arrays]


def _unknown_mask(H, W, mask):
    m = torch.zeros((H, W), dtype=torch.bool, device='cuda')
    si, sj = BT.unknown_slices(H, W, mask)
    m[si, sj] = True
    return m


@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=lambda s: '%dx%d' % s)
def test_loss_sums_and_gradient_against_the_twin(ops, shape):
    H, W = shape
    u, rho, rhs, g, dx, coef = _case(H, W)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)
    worst_sum = worst_grad = 0.0
    for mask in ALL_MASKS:
        got = ops.varcoef_pi_loss_partials(du, drho, drhs, ddx, mask).cpu().double().numpy()
        ref = BT.loss_batch(u, rho, rhs, dx, mask)
        rel = float((np.abs(got - ref) / ref).max())
        grad = ops.varcoef_pi_loss_bwd(du, drho, drhs, ddx, dcoef, torch.zeros_like(du), mask)
        grel = BT.rel_l2(grad.cpu().numpy(), BT.loss_grad_batch(u, rho, rhs, dx, mask, coef))
        worst_sum, worst_grad = max(worst_sum, rel), max(worst_grad, grel)
        assert rel <= SUM_TOL and grel <= FIELD_TOL, (mask, rel, grel)
        # it adds into what dpred holds: one fp32 addition per node on top of the same product
        assert torch.equal(ops.varcoef_pi_loss_bwd(du, drho, drhs, ddx, dcoef, dg.clone(), mask), dg + grad), mask
        # flags name the same mask
        assert torch.equal(ops.varcoef_pi_loss_partials(du, drho, drhs, ddx, B.flags(mask)), torch.tensor(got, device='cuda', dtype=torch.float32)), mask
    print('loss %d x %d, 16 masks: sums max relative error %.3g, dpred max rel-L2 %.3g' % (H, W, worst_sum, worst_grad))


@functools.lru_cache(maxsize=None)
def _sweep_matrices(H, W, mask):
    u, rho, rhs, g, dx, _ = _case(H, W)
    return [BT.sweep_matrix(rho[n], float(dx[n]), mask) for n in range(N)]


@pytest.mark.parametrize('mask', SWEEP_MASKS)
@pytest.mark.parametrize('shape', SWEEP_SHAPES, ids=lambda s: '%dx%d' % s)
def test_sweeps_and_adjoint_against_the_twin(ops, shape, mask):
    H, W = shape
    u, rho, rhs, g, dx, _ = _case(H, W)
    du, drho, drhs, dg, ddx = _dev(u, rho, rhs, g, dx)
    mats = _sweep_matrices(H, W, mask)
    unknown = _unknown_mask(H, W, mask)
    zero = torch.zeros_like(du)
    fwd = [u[n].ravel().copy() for n in range(N)]
    adj = [g[n].ravel().copy() for n in range(N)]
    done = 0
    for n_sweeps in SWEEP_COUNTS:
        for n in range(N):
            J, scale = mats[n]
            c, Jt = scale * rhs[n].ravel(), J.T.tocsr()
            for _ in range(n_sweeps - done):
                fwd[n] = J @ fwd[n] - c
                adj[n] = Jt @ adj[n]
        done = n_sweeps
        out = ops.varcoef_jacobi(du, drho, drhs, ddx, n_sweeps, mask)
        back = ops.varcoef_jacobi_bwd(dg, drho, ddx, n_sweeps, mask)
        rel = BT.rel_l2(out.cpu().numpy(), np.stack(fwd).reshape(N, H, W))
        rel_adj = BT.rel_l2(back.cpu().numpy(), np.stack(adj).reshape(N, H, W))
        # <J^T g, v> = <g, J v - J 0>, both sides from the kernels, summed in fp64 - with v = |u| and g = |g|: J has no negative entry, so neither
        # side cancels and "relative to the inner product" measures the kernels, not a sum of random signs that happens to come out near zero
        # (with u and g themselves one draw gave an inner product 1e-5 of |g| |J v|, where fp32 rounding of the fields alone is 3e-5 of it)
        lin = ops.varcoef_jacobi(du.abs(), drho, drhs, ddx, n_sweeps, mask).double() - ops.varcoef_jacobi(zero, drho, drhs, ddx, n_sweeps, mask).double()
        lhs = float((ops.varcoef_jacobi_bwd(dg.abs(), drho, ddx, n_sweeps, mask).double() * du.abs().double()).sum())
        rhs_ = float((dg.abs().double() * lin).sum())
        print('jacobi %d x %d mask %d, %d sweeps: forward rel-L2 %.3g, adjoint %.3g, identity %.3g of the inner product'
              % (H, W, mask, n_sweeps, rel, rel_adj, abs(lhs - rhs_) / abs(rhs_)))
        assert rel <= FIELD_TOL and rel_adj <= FIELD_TOL
        assert abs(lhs - rhs_) <= DOT_TOL * abs(rhs_), (lhs, rhs_)
        # Dirichlet nodes are frozen bit for bit; every unknown moved - the nodes of the Neumann edges among them
        assert torch.equal(out[:, ~unknown], du[:, ~unknown])
        assert bool((out[:, unknown] != du[:, unknown]).all())
        for bit, edge in enumerate((out[:, 0, 1:-1], out[:, -1, 1:-1], out[:, 1:-1, 0], out[:, 1:-1, -1])):
            same = edge == (du[:, 0, 1:-1], du[:, -1, 1:-1], du[:, 1:-1, 0], du[:, 1:-1, -1])[bit]
            assert bool(same.all()) if not (mask >> bit & 1) else not bool(same.any()), (mask, bit)


def test_mask_0_through_the_new_entry_points_is_the_old_kernels(ops):
    """pcnn_varcoef_bc_* with neumann_mask 0 called directly (ops.* route a zero mask to the old names): the same bits for all four operators."""
    H, W = 19, 70
    u, rho, rhs, g, dx, coef = _case(H, W)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)
    p, ci, call = ops._p, ctypes.c_int, ops.handle().call
    out = torch.empty(N, device='cuda')
    call('pcnn_varcoef_bc_pi_loss_partials', ci(N), ci(H), ci(W), p(du), p(drho), p(drhs), p(ddx), p(out), ci(0))
    assert torch.equal(out, ops.varcoef_pi_loss_partials(du, drho, drhs, ddx))
    grad = dg.clone()
    call('pcnn_varcoef_bc_pi_loss_bwd', ci(N), ci(H), ci(W), p(du), p(drho), p(drhs), p(ddx), p(dcoef), p(grad), ci(0))
    assert torch.equal(grad, ops.varcoef_pi_loss_bwd(du, drho, drhs, ddx, dcoef, dg.clone()))
    for n_sweeps in (3, 9):
        y = torch.empty_like(du)
        call('pcnn_varcoef_bc_jacobi_fwd', ci(N), ci(H), ci(W), p(drho), p(du), p(drhs), p(ddx), ci(n_sweeps), p(y), ci(0))
        assert torch.equal(y, ops.varcoef_jacobi(du, drho, drhs, ddx, n_sweeps))
        call('pcnn_varcoef_bc_jacobi_bwd', ci(N), ci(H), ci(W), p(drho), p(ddx), p(dg), ci(n_sweeps), p(y), ci(0))
        assert torch.equal(y, ops.varcoef_jacobi_bwd(dg, drho, ddx, n_sweeps))


@pytest.mark.parametrize('mask', [5, 15])
def test_two_runs_are_bit_equal_and_a_sample_does_not_see_its_batch(ops, mask):
    u, rho, rhs, g, dx, coef = _case(66, 130)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)

    def run(s):
        a = [t[s].contiguous() for t in (du, drho, drhs, dg, ddx, dcoef)]
        return (ops.varcoef_pi_loss_partials(a[0], a[1], a[2], a[4], mask), ops.varcoef_pi_loss_bwd(a[0], a[1], a[2], a[4], a[5], torch.zeros_like(a[0]), mask),
                ops.varcoef_jacobi(a[0], a[1], a[2], a[4], 9, mask), ops.varcoef_jacobi_bwd(a[3], a[1], a[4], 9, mask))
    first, second, alone = run(slice(0, 3)), run(slice(0, 3)), run(slice(1, 2))
    for a, b, c in zip(first, second, alone):
        assert torch.equal(a, b) and torch.equal(a[1:2], c)


@pytest.mark.parametrize('mask', [5, 15])
def test_generator_solution_is_a_fixed_point_of_the_neumann_sweeps(ops, mask):
    """variable_density_dataset_generator(boundary_types=...) - the solve of DESIGN.md section 19, for mask 15 with the projected right-hand side -
    under 8 sweeps with the same mask: fp32 rounding on an fp32-rounded fixed point (1e-5, the bound of the Dirichlet counterpart in
    tests/test_gpu_varcoef_train.py).  That the mask matters shows under the sweeps of another mask: the solution of mask 5 under those of mask 10
    (the other two edges Neumann) moves by more than the bound.  Sweeps with every edge frozen (mask 0) can NOT show it: the interior rows are the
    same for every mask and the frozen edge nodes hold the solution's own values, so the solution is a fixed point of those too (measured on an
    MI355X: 1.1e-7 frozen against 1.2e-7 with the mask)."""
    from poisson_cnn_amd import dataset as D
    gen = D.variable_density_dataset_generator(batch_size=2, output_shape=(33, 47), seed=3, boundary_types=B.types(mask))
    (stack, dx), soln = gen[0]
    rhs, rho, u, d = stack[:, 0].contiguous(), stack[:, 1].contiguous(), soln[:, 0].contiguous(), dx.reshape(-1).contiguous()
    rel = BT.rel_l2(ops.varcoef_jacobi(u, rho, rhs, d, 8, mask).cpu().numpy(), u.cpu().numpy())
    frozen = BT.rel_l2(ops.varcoef_jacobi(u, rho, rhs, d, 8, 0).cpu().numpy(), u.cpu().numpy())
    other = BT.rel_l2(ops.varcoef_jacobi(u, rho, rhs, d, 8, 10).cpu().numpy(), u.cpu().numpy())
    print('generator solution, mask %d, under 8 sweeps: moves by rel-L2 %.3g with the mask, %.3g with every edge frozen, %.3g under mask 10'
          % (mask, rel, frozen, other))
    assert rel <= 1e-5 and frozen <= 1e-5
    if mask == 5:
        assert other > 1e-5


def test_c_abi_refusals(ops):
    u, rho, rhs, g, dx, coef = _case(3, 4)
    du, drho, drhs, dg, ddx, dcoef = _dev(u, rho, rhs, g, dx, coef)
    p, ci, call = ops._p, ctypes.c_int, ops.handle().call
    out, y = torch.empty(N, device='cuda'), torch.empty_like(du)
    for bad in (16, -1):
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_pi_loss_partials', ci(N), ci(3), ci(4), p(du), p(drho), p(drhs), p(ddx), p(out), ci(bad))
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_pi_loss_bwd', ci(N), ci(3), ci(4), p(du), p(drho), p(drhs), p(ddx), p(dcoef), p(y), ci(bad))
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_jacobi_fwd', ci(N), ci(3), ci(4), p(drho), p(du), p(drhs), p(ddx), ci(1), p(y), ci(bad))
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_jacobi_bwd', ci(N), ci(3), ci(4), p(drho), p(ddx), p(dg), ci(1), p(y), ci(bad))
        with pytest.raises(ValueError, match='neumann_mask'):
            ops.varcoef_jacobi(du, drho, drhs, ddx, 1, bad)
    with pytest.raises(RuntimeError, match='unsupported'):             # H = 2
        call('pcnn_varcoef_bc_pi_loss_partials', ci(N), ci(2), ci(6), p(du), p(drho), p(drhs), p(ddx), p(out), ci(5))
    with pytest.raises(RuntimeError, match='H, W >= 3'):
        call('pcnn_varcoef_bc_jacobi_fwd', ci(N), ci(2), ci(6), p(drho), p(du), p(drhs), p(ddx), ci(1), p(y), ci(5))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_pi_loss_bwd', ci(N), ci(3), ci(4), p(du), p(drho), p(drhs), p(ddx), p(dcoef), p(du), ci(5))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_jacobi_fwd', ci(N), ci(3), ci(4), p(drho), p(du), p(drhs), p(ddx), ci(1), p(du), ci(5))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_jacobi_bwd', ci(N), ci(3), ci(4), p(drho), p(ddx), p(dg), ci(1), p(dg), ci(5))
    with pytest.raises(ValueError, match='four flags'):
        ops.varcoef_jacobi(du, drho, drhs, ddx, 1, (True, False))
