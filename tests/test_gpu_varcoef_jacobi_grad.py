"""The variable-density smoother's gradients w.r.t. u, rho and rhs (pcnn_varcoef_bc_jacobi_bwd_inputs of csrc/varcoef_train.hip,
ops.varcoef_jacobi_bwd_inputs, autograd.variable_density_smooth) against the float64 twin of tests/varcoef_jacobi_grad_twin.py
(pinned by tests/test_varcoef_jacobi_grad_reference.py) fed the same fp32 inputs.

Shapes: 3 x 3 (one unknown at mask 0), 4 x 5, 16 x 64 and 17 x 65 (either side of the 16 x 64 tile), 19 x 70 (past the tile by more than a halo) and
33 x 130 (tiles in both directions, a ragged last one); N = 3 with a different dx per sample; rho random with a 100 : 1 jump along the diagonal of the
field, which crosses every tile boundary; 1, 2 and k_max + 1 sweeps - the last chains launches in the forward and in the fused adjoint.
Bound: 4 x FLOOR, as section 24's fp32 kernels have it: FLOOR is the error of the twin's same closed-form formulas evaluated in float32 on the CPU
on the same inputs - per shape, sweep count and output the worst of the masks, which differ only in which nodes are unknowns; the factor covers
the summation order and the association of the products (the kernel forms (1 / D) g where the twin forms g / D).
Run with -s for the measured figures (DESIGN.md section 25 holds a copy)."""
import ctypes

import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_jacobi_grad_twin as J

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3), (4, 5), (16, 64), (17, 65), (19, 70), (33, 130)]
MASKS = [0, 1, 6, 9, 15]
N = 3
SUBSETS = [('u',), ('rho',), ('rhs',), ('u', 'rho'), ('u', 'rhs'), ('rho', 'rhs')]


@pytest.fixture(scope='module')
def ops():
    from poisson_cnn_amd import ops
    return ops


def _dev(a):
    return torch.tensor(a, device='cuda', dtype=torch.float32).contiguous()


def _sweeps(ops):
    return [1, 2, ops.varcoef_jacobi_k_max() + 1]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_gradients_against_the_twin(ops, shape):
    H, W = shape
    u, rho, rhs, gbar, dx = J.case(H, W, N)
    d_u, d_rho, d_rhs, d_g, d_dx = _dev(u), _dev(rho), _dev(rhs), _dev(gbar), _dev(dx)
    for n_sweeps in _sweeps(ops):
        errs, floors = {}, dict.fromkeys(J.KEYS, 0.0)
        for mask in MASKS:
            ref, floor = J.reference(H, W, mask, n_sweeps, N)
            got = dict(zip(J.KEYS, ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, n_sweeps, mask)))
            for k in J.KEYS:
                errs[mask, k] = J.rel_l2(got[k].cpu(), ref[k])
                floors[k] = max(floors[k], floor[k])
            # du has the bits of the fused adjoint, whose launches split the sweeps differently
            assert torch.equal(got['u'], ops.varcoef_jacobi_bwd(d_g, d_rho, d_dx, n_sweeps, mask)), (mask, n_sweeps)
            # rhs is read on the unknowns only
            assert not bool(got['rhs'].cpu()[:, ~J.unknown_mask(H, W, mask)].any())
            # gathers without atomics: a second run gives the same bits (the scratch is reused in between)
            for a, b in zip(got.values(), ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, n_sweeps, mask)):
                assert torch.equal(a, b), (mask, n_sweeps)
            # a `want` subset returns only what was asked, with the bits of the full call
            for want in SUBSETS:
                part = dict(zip(J.KEYS, ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, n_sweeps, mask, want=want)))
                for k in J.KEYS:
                    assert (part[k] is None) if k not in want else torch.equal(part[k], got[k]), (mask, n_sweeps, want, k)
        for k in J.KEYS:
            worst = max(errs[m, k] for m in MASKS)
            print('jacobi_bwd_inputs %d x %d, %d sweeps, d%s: worst rel-L2 %.3g, fp32 floor of the twin %.3g (ratio %.2f)'
                  % (H, W, n_sweeps, k, worst, floors[k], worst / floors[k]))
        for (mask, k), e in errs.items():
            assert e <= 4.0 * floors[k], (n_sweeps, mask, k, e, floors[k])
    # four flags name the same mask
    assert torch.equal(ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, 2, B.flags(6))[1], ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, 2, 6)[1])


@pytest.mark.parametrize('mask', [0, 9])
def test_smooth_on_the_tape(ops, mask):
    from poisson_cnn_amd import autograd
    H, W, n_sweeps = 17, 65, 2
    u, rho, rhs, gbar, dx = J.case(H, W, N)
    d_g, d_dx = _dev(gbar), _dev(dx)
    leaves = {k: _dev(a).reshape(N, 1, H, W).requires_grad_(True) for k, a in zip(J.KEYS, (u, rho, rhs))}
    out = autograd.variable_density_smooth(leaves['u'], leaves['rho'], leaves['rhs'], d_dx.reshape(N, 1), n_sweeps, boundary_types=B.types(mask))
    plain = [leaves[k].detach().reshape(N, H, W) for k in J.KEYS]
    assert out.shape == (N, 1, H, W) and out.grad_fn is not None
    assert torch.equal(out.detach().reshape(N, H, W), ops.varcoef_jacobi(*plain, d_dx, n_sweeps, mask))
    (out[:, 0] * d_g).sum().backward()
    want = ops.varcoef_jacobi_bwd_inputs(d_g, *plain, d_dx, n_sweeps, mask)
    for k, g in zip(J.KEYS, want):
        assert leaves[k].grad.shape == (N, 1, H, W) and torch.equal(leaves[k].grad.reshape(N, H, W), g), k
    # .grad only on the inputs that require it; two equal columns of dx are one spacing
    for needs in (('rho',), ('u', 'rhs')):
        t = {k: _dev(a).requires_grad_(k in needs) for k, a in zip(J.KEYS, (u, rho, rhs))}
        res = autograd.variable_density_smooth(t['u'], t['rho'], t['rhs'], torch.stack([d_dx, d_dx], dim=1), n_sweeps, boundary_types=B.types(mask))
        assert res.shape == (N, H, W)
        (res * d_g).sum().backward()
        for k, g in zip(J.KEYS, want):
            assert (t[k].grad is None) if k not in needs else torch.equal(t[k].grad, g), (needs, k)
    # nothing requires grad, or no_grad: the forward alone, no graph
    assert autograd.variable_density_smooth(*plain, d_dx, n_sweeps, boundary_types=B.types(mask)).grad_fn is None
    with torch.no_grad():
        assert autograd.variable_density_smooth(leaves['u'], leaves['rho'], leaves['rhs'], d_dx, n_sweeps, boundary_types=B.types(mask)).grad_fn is None


def test_smooth_into_the_residual_backpropagates_to_rho():
    """variable_density_smooth -> variable_density_residual at 17 x 65, mask 9: rho feeds both; FLOOR is the twin's chain evaluated in float32."""
    from poisson_cnn_amd import autograd
    H, W, n_sweeps, mask = 17, 65, 2, 9
    u, rho, rhs, _, dx = J.case(H, W, N)
    coef = [0.7 * float(d) ** 4 for d in dx]
    t = {k: _dev(a).requires_grad_(True) for k, a in zip(J.KEYS, (u, rho, rhs))}
    d_dx = _dev(dx)
    pred = autograd.variable_density_smooth(t['u'], t['rho'], t['rhs'], d_dx, n_sweeps, boundary_types=B.types(mask))
    out = autograd.variable_density_residual(pred, torch.stack([t['rhs'], t['rho']], dim=1), d_dx, boundary_types=B.types(mask))
    (out * _dev(coef)).sum().backward()
    ref = [J.chain_closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, coef[n]) for n in range(N)]
    low = [J.chain_closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, coef[n], dtype=torch.float32) for n in range(N)]
    figures = {}
    for k in J.KEYS:
        r = torch.stack([g[k] for g in ref])
        figures[k] = (J.rel_l2(t[k].grad.cpu(), r), J.rel_l2(torch.stack([g[k] for g in low]), r))
        print('smooth -> residual 17 x 65 mask 9 d%s: rel-L2 %.3g, fp32 floor of the twin %.3g (ratio %.2f)' % ((k,) + figures[k] + (figures[k][0] / figures[k][1],)))
    for k, (err, floor) in figures.items():
        assert err <= 4.0 * floor, (k, err, floor)


def test_smooth_composes_with_the_solve():
    """variable_density_solve -> variable_density_smooth: a smoothing of the solution changes it little, and rho gets a gradient from both."""
    from poisson_cnn_amd import autograd
    H, W = 17, 65
    u, rho, rhs, gbar, dx = J.case(H, W, N)
    d_rho = (_dev(rho) / 50.0).clamp(1.0, 2.0).requires_grad_(True)
    d_rhs, d_dx = _dev(rhs), _dev(dx)
    edges = {k: torch.zeros(N, W if k in ('left', 'right') else H, device='cuda') for k in B.EDGES}
    soln = autograd.variable_density_solve(d_rho, d_rhs, edges, d_dx, tol=1e-12)
    out = autograd.variable_density_smooth(soln, d_rho, d_rhs, d_dx, 2)
    assert out.shape == soln.shape and float((out - soln).detach().norm() / soln.detach().norm()) < 1e-3       # the solution is the sweep's fixed point
    (out[:, 0] * _dev(gbar)).sum().backward()
    assert d_rho.grad is not None and bool(torch.isfinite(d_rho.grad).all()) and float(d_rho.grad.abs().max()) > 0.0


def test_refusals(ops):
    from poisson_cnn_amd import autograd
    H, W = 4, 5
    u, rho, rhs, gbar, dx = J.case(H, W, N)
    d_u, d_rho, d_rhs, d_g, d_dx = _dev(u), _dev(rho), _dev(rhs), _dev(gbar), _dev(dx)
    for bad in (0, -1):
        with pytest.raises(ValueError, match='n_sweeps'):
            ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, bad)
        with pytest.raises(ValueError, match='n_sweeps'):
            autograd.variable_density_smooth(d_u, d_rho, d_rhs, d_dx, bad)
    for bad in (16, -1):
        with pytest.raises(ValueError, match='neumann_mask'):
            ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, 1, bad)
    with pytest.raises(ValueError, match='float32'):
        ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho.double(), d_rhs, d_dx, 1)
    with pytest.raises(ValueError, match='float32'):
        ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs.cpu(), d_dx, 1)
    with pytest.raises(ValueError, match='float32'):
        autograd.variable_density_smooth(d_u, d_rho.double(), d_rhs, d_dx, 1)
    with pytest.raises(ValueError, match='device'):
        autograd.variable_density_smooth(d_u.cpu(), d_rho, d_rhs, d_dx, 1)
    with pytest.raises(ValueError, match='want'):
        ops.varcoef_jacobi_bwd_inputs(d_g, d_u, d_rho, d_rhs, d_dx, 1, want=('dx',))
    with pytest.raises(NotImplementedError, match='anisotropic'):
        autograd.variable_density_smooth(d_u, d_rho, d_rhs, torch.stack([d_dx, 2.0 * d_dx], dim=1), 1)
    # the C ABI's own checks
    p, ci, call = ops._p, ctypes.c_int, ops.handle().call
    y, z = torch.empty_like(d_u), torch.empty_like(d_u)
    args = lambda mask, n_sweeps, du, drho, drhs, h=H: (ci(N), ci(h), ci(W), ci(mask), p(d_rho), p(d_u), p(d_rhs), p(d_dx), p(d_g), ci(n_sweeps), p(du), p(drho), p(drhs))
    for bad in (16, -1):
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(bad, 1, y, z, None))
    with pytest.raises(RuntimeError, match='n_sweeps'):
        call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(0, 0, y, z, None))
    with pytest.raises(RuntimeError, match='n_sweeps'):
        call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(0, 1, y, z, None, h=2))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(0, 1, y, d_u, None))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(0, 1, None, y, y))
    with pytest.raises(RuntimeError, match='null'):
        call('pcnn_varcoef_bc_jacobi_bwd_inputs', ci(N), ci(H), ci(W), ci(0), p(d_rho), p(None), p(d_rhs), p(d_dx), p(d_g), ci(1), p(y), p(None), p(None))
    call('pcnn_varcoef_bc_jacobi_bwd_inputs', *args(0, 1, None, None, None))             # nothing wanted: nothing done
