"""The gradients of the variable-density problem with respect to its data (csrc/varcoef_grad.hip, autograd.variable_density_solve /
variable_density_residual) against the float64 twin of tests/varcoef_grad_twin.py (pinned by
tests/test_varcoef_grad_reference.py) fed the same fp32 inputs.

Shapes: 3 x 3 (one unknown at mask 0), 4 x 5, 16 x 64 and 17 x 65 (either side of the 16 x 64 tile), 19 x 70 (past the tile by more than a halo) and
33 x 130 (tiles in both directions, a ragged last one); a different dx per sample; rho random with a 100 : 1 jump along the diagonal of the field,
which crosses every tile boundary.  Bounds:
  * coef_grad / edge_grad: rel-L2 2e-6 per output over the batch, the project's per-operator bound (fp64 sums of fp32 inputs, one rounding);
  * pi_loss_bwd_inputs (fp32 throughout): 4 x FLOOR, where FLOOR is the error of the twin's same closed-form formulas evaluated in float32 on the
    CPU on the same inputs - per shape and output the worst of the masks, which differ only in which nodes are unknowns; the factor covers the
    summation order and the association of the products;
  * the solve's backward: 4 x FLOOR, FLOOR the error of the twin's formulas with ITS lam and u rounded to float32 - what handing a converged fp64
    solve over in fp32 costs - per mask and output.
Run with -s for the measured figures (DESIGN.md section 24 holds a copy)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_grad_twin as G

pytestmark = pytest.mark.gpu

OP_TOL = 2e-6
SHAPES = [(3, 3), (4, 5), (16, 64), (17, 65), (19, 70), (33, 130)]
MASKS = [0, 1, 2, 4, 8, 6, 9, 15]
SOLVE_MASKS = [0, 1, 6, 9]
KEYS = ('rho', 'rhs') + B.EDGES


@pytest.fixture(scope='module')
def ops():
    from poisson_cnn_amd import ops
    return ops


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _jump_density(rng, N, H, W, lo=1.0, hi=2.0, ratio=100.0):
    rho = rng.uniform(lo, hi, (N, H, W))
    below = (np.arange(H)[:, None] * (W - 1)) > (np.arange(W)[None, :] * (H - 1))
    rho[:, below] *= ratio
    return rho


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """fp32-rounded host arrays (read-only), float64: u, lam0 (to be zeroed off the unknowns), rho, rhs, du (N,H,W), edges dict, dx, coef (N,)."""
    N = 3 if H * W <= 20 else 2
    rng = np.random.default_rng(3000 * H + W)
    u, lam0, rhs, du = (_f32(rng.standard_normal((N, H, W))) for _ in range(4))
    rho = _f32(_jump_density(rng, N, H, W))
    edges = {k: _f32(rng.standard_normal((N, W if k in ('left', 'right') else H))) for k in B.EDGES}
    dx = _f32(rng.uniform(5e-3, 5e-2, N))
    coef = _f32(rng.uniform(0.5, 2.0, N) * float(dx.min()) ** 4)
    for a in (u, lam0, rho, rhs, du, dx, coef) + tuple(edges.values()):
        a.setflags(write=False)
    return u, lam0, rho, rhs, du, edges, dx, coef


def _dev(a):
    return torch.tensor(np.asarray(a), device='cuda', dtype=torch.float32).contiguous()


def _stack(dicts, key):
    return torch.stack([d[key] for d in dicts])


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_coef_and_edge_gradients_against_the_twin(ops, shape):
    H, W = shape
    u, lam0, rho, rhs, du, edges, dx, _ = _case(H, W)
    N = u.shape[0]
    d_u, d_rho, d_du, d_dx = _dev(u), _dev(rho), _dev(du), _dev(dx)
    d_edges = {k: _dev(v) for k, v in edges.items()}
    worst = 0.0
    for mask in MASKS:
        lam = lam0 * G.unknown_mask(H, W, mask).numpy()
        d_lam = _dev(lam)
        for with_data in (True, False):
            ref = [G.closed_form(lam[n], u[n], rho[n], dx[n], mask, {k: v[n] for k, v in edges.items()} if with_data else None, du[n] if with_data else None)
                   for n in range(N)]
            drho = ops.varcoef_coef_grad(d_lam, d_u, d_rho, d_dx, mask, d_edges if with_data else None)
            dedges = ops.varcoef_edge_grad(d_lam, d_rho, d_dx, mask, d_du if with_data else None)
            got = dict(zip(('rho',) + B.EDGES, (drho,) + tuple(dedges)))
            for k, g in got.items():
                err = G.rel_l2(g.cpu(), _stack(ref, k))
                worst = max(worst, err)
                assert err <= OP_TOL, (mask, with_data, k, err)
            # gathers without atomics: a second run gives the same bits
            assert torch.equal(drho, ops.varcoef_coef_grad(d_lam, d_u, d_rho, d_dx, mask, d_edges if with_data else None)), mask
            for a, b in zip(dedges, ops.varcoef_edge_grad(d_lam, d_rho, d_dx, mask, d_du if with_data else None)):
                assert torch.equal(a, b), mask
        # four flags name the same mask; a Dirichlet edge's array is not read as Neumann data
        assert torch.equal(ops.varcoef_coef_grad(d_lam, d_u, d_rho, d_dx, B.flags(mask), d_edges), ops.varcoef_coef_grad(d_lam, d_u, d_rho, d_dx, mask, d_edges))
    print('coef_grad / edge_grad %d x %d, %d masks, with and without data: worst rel-L2 %.3g (bound %.3g)' % (H, W, len(MASKS), worst, OP_TOL))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_fused_loss_gradients_against_the_twin(ops, shape):
    H, W = shape
    u, _, rho, rhs, _, _, dx, coef = _case(H, W)
    N = u.shape[0]
    d_u, d_rho, d_rhs, d_dx, d_coef = _dev(u), _dev(rho), _dev(rhs), _dev(dx), _dev(coef)
    errs, floors = {}, {'rhs': 0.0, 'rho': 0.0}
    for mask in MASKS:
        ref = [G.loss_closed_form(u[n], rho[n], rhs[n], dx[n], mask, coef[n])[1] for n in range(N)]
        low = [G.loss_closed_form(u[n], rho[n], rhs[n], dx[n], mask, coef[n], dtype=torch.float32)[1] for n in range(N)]
        drhs, drho = ops.varcoef_pi_loss_bwd_inputs(d_u, d_rho, d_rhs, d_dx, d_coef, mask)
        for k, g in (('rhs', drhs), ('rho', drho)):
            errs[mask, k] = G.rel_l2(g.cpu(), _stack(ref, k))
            floors[k] = max(floors[k], G.rel_l2(_stack(low, k), _stack(ref, k)))
        # rhs is read on the unknowns only
        assert not bool(drhs.cpu()[:, ~G.unknown_mask(H, W, mask)].any())
        # `want` subsets write only what was asked, with the same bits; two runs agree
        only_rhs, only_rho = ops.varcoef_pi_loss_bwd_inputs(d_u, d_rho, d_rhs, d_dx, d_coef, mask, want=('rhs',)), \
            ops.varcoef_pi_loss_bwd_inputs(d_u, d_rho, d_rhs, d_dx, d_coef, mask, want=('rho',))
        assert only_rhs[1] is None and only_rho[0] is None and torch.equal(only_rhs[0], drhs) and torch.equal(only_rho[1], drho)
    for k in ('rhs', 'rho'):
        worst = max(errs[m, k] for m in MASKS)
        print('pi_loss_bwd_inputs %d x %d d%s: worst rel-L2 %.3g, fp32 floor of the twin %.3g (ratio %.2f)' % (H, W, k, worst, floors[k], worst / floors[k]))
    for (mask, k), e in errs.items():
        assert e <= 4.0 * floors[k], (mask, k, e, floors[k])
    with pytest.raises(ValueError, match='want'):
        ops.varcoef_pi_loss_bwd_inputs(d_u, d_rho, d_rhs, d_dx, d_coef, 0, want=('pred',))


# ----------------------------------------------------------------------------- the differentiable solve
SOLVE_SHAPE, SOLVE_N = (19, 70), 2


@functools.lru_cache(maxsize=None)
def _solve_case():
    H, W = SOLVE_SHAPE
    rng = np.random.default_rng(77)
    rho = _f32(rng.uniform(1.0, 3.0, (SOLVE_N, H, W)))
    rhs, wts = _f32(rng.standard_normal((SOLVE_N, H, W))), _f32(rng.standard_normal((SOLVE_N, H, W)))
    edges = {k: _f32(rng.standard_normal((SOLVE_N, W if k in ('left', 'right') else H))) for k in B.EDGES}
    dx = _f32(rng.uniform(1e-2, 5e-2, SOLVE_N))
    return rho, rhs, edges, dx, wts


@functools.lru_cache(maxsize=None)
def _solve_reference(mask):
    """Per mask, once: the twin's gradients by autograd through the dense solve, and the floor - its closed form with lam and u rounded to fp32."""
    rho, rhs, edges, dx, wts = _solve_case()
    H, W = SOLVE_SHAPE
    auto, low = [], []
    for n in range(SOLVE_N):
        e = {k: v[n] for k, v in edges.items()}
        u, g = G.solve_grads(rho[n], rhs[n], e, dx[n], mask, wts[n])
        lam = G.adjoint(rho[n], dx[n], mask, wts[n])
        auto.append(g)
        low.append(G.closed_form(lam.to(torch.float32).to(torch.float64), u.to(torch.float32).to(torch.float64), rho[n], dx[n], mask, e, wts[n]))
    return {k: _stack(auto, k) for k in KEYS}, {k: G.rel_l2(_stack(low, k), _stack(auto, k)) for k in KEYS}


def _solve_inputs(requires=KEYS):
    rho, rhs, edges, dx, wts = _solve_case()
    t = {'rho': _dev(rho), 'rhs': _dev(rhs), **{k: _dev(v) for k, v in edges.items()}}
    for k in requires:
        t[k].requires_grad_(True)
    return t, _dev(dx), _dev(wts)


@pytest.mark.parametrize('preconditioner', ['dst', 'scaled'])
@pytest.mark.parametrize('mask', SOLVE_MASKS)
def test_solve_forward_bits_and_gradients_against_the_twin(mask, preconditioner):
    from poisson_cnn_amd import autograd, dataset as D
    t, dx, wts = _solve_inputs()
    H, W = SOLVE_SHAPE
    kw = dict(boundary_types=B.types(mask), tol=1e-12, max_iterations=500, preconditioner=preconditioner)
    edges = {k: t[k] for k in B.EDGES}
    u = autograd.variable_density_solve(t['rho'], t['rhs'], edges, dx, **kw)
    assert u.shape == (SOLVE_N, 1, H, W) and u.dtype == torch.float32 and u.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(u, D.variable_density_poisson_solve(t['rho'], t['rhs'], edges, dx, **kw))
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                # an adjoint solve that has not converged would warn
        (u[:, 0] * wts).sum().backward()
    ref, floor = _solve_reference(mask)
    for k in KEYS:
        err = G.rel_l2(t[k].grad.cpu(), ref[k])
        print('solve 19 x 70 mask %d %s d%s: rel-L2 %.3g, floor of an fp32 hand-over %.3g (ratio %.2f)' % (mask, preconditioner, k, err, floor[k], err / floor[k]))
    for k in KEYS:
        assert G.rel_l2(t[k].grad.cpu(), ref[k]) <= 4.0 * floor[k], (k, G.rel_l2(t[k].grad.cpu(), ref[k]), floor[k])


def test_solve_runs_nothing_it_was_not_asked_for(monkeypatch):
    from poisson_cnn_amd import autograd
    from poisson_cnn_amd.dataset import _kernels as K
    calls = []
    real = K.varcoef_pcg_solve
    monkeypatch.setattr(K, 'varcoef_pcg_solve', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    kw = dict(boundary_types=B.types(6), tol=1e-12)
    # only rho and one edge require grad: the others get None, and the backward is one more solve
    t, dx, wts = _solve_inputs(requires=('rho', 'top'))
    u = autograd.variable_density_solve(t['rho'], t['rhs'], {k: t[k] for k in B.EDGES}, dx, **kw)
    assert len(calls) == 1
    (u[:, 0] * wts).sum().backward()
    assert len(calls) == 2
    assert t['rho'].grad is not None and t['top'].grad is not None
    assert all(t[k].grad is None for k in ('rhs', 'left', 'right', 'bottom'))
    ref, floor = _solve_reference(6)
    assert G.rel_l2(t['rho'].grad.cpu(), ref['rho']) <= 4.0 * floor['rho'] and G.rel_l2(t['top'].grad.cpu(), ref['top']) <= 4.0 * floor['top']
    # nothing requires grad, or no_grad: the forward solve alone, no graph
    del calls[:]
    t2, _, _ = _solve_inputs(requires=())
    assert autograd.variable_density_solve(t2['rho'], t2['rhs'], {k: t2[k] for k in B.EDGES}, dx, **kw).grad_fn is None
    with torch.no_grad():
        v = autograd.variable_density_solve(t['rho'], t['rhs'], {k: t[k] for k in B.EDGES}, dx, **kw)
    assert v.grad_fn is None and not v.requires_grad and len(calls) == 2 and torch.equal(v, u)


def test_solve_refusals():
    from poisson_cnn_amd import autograd
    t, dx, _ = _solve_inputs(requires=('rho',))
    edges = {k: t[k] for k in B.EDGES}
    with pytest.raises(NotImplementedError, match='all-Neumann'):
        autograd.variable_density_solve(t['rho'], t['rhs'], edges, dx, boundary_types=B.types(15))
    two = torch.stack([dx, 2.0 * dx], dim=1).contiguous()
    with pytest.raises(NotImplementedError, match='anisotropic'):
        autograd.variable_density_solve(t['rho'], t['rhs'], edges, two)
    with pytest.raises(ValueError, match='lacks'):
        autograd.variable_density_solve(t['rho'], t['rhs'], {k: t[k] for k in ('left', 'right')}, dx)


@pytest.mark.parametrize('mask', [0, 9, 15])
def test_residual_on_the_tape(ops, mask):
    from poisson_cnn_amd import autograd
    H, W = 19, 70
    u, _, rho, rhs, _, _, dx, coef = _case(H, W)
    N = u.shape[0]
    pred = _dev(u).reshape(N, 1, H, W).requires_grad_(True)
    stack = torch.stack([_dev(rhs), _dev(rho)], dim=1).contiguous().requires_grad_(True)
    d_dx, d_coef = _dev(dx), _dev(coef)
    out = autograd.variable_density_residual(pred, stack, d_dx.reshape(N, 1), boundary_types=B.types(mask))
    p, f, r = pred.detach().reshape(N, H, W), stack.detach()[:, 0].contiguous(), stack.detach()[:, 1].contiguous()
    assert out.shape == (N,) and torch.equal(out, ops.varcoef_pi_loss_partials(p, r, f, d_dx, mask))
    (out * d_coef).sum().backward()
    assert torch.equal(pred.grad.reshape(N, H, W), ops.varcoef_pi_loss_bwd(p, r, f, d_dx, d_coef, torch.zeros_like(p), mask))
    ref = [G.loss_closed_form(u[n], rho[n], rhs[n], dx[n], mask, coef[n])[1] for n in range(N)]
    low = [G.loss_closed_form(u[n], rho[n], rhs[n], dx[n], mask, coef[n], dtype=torch.float32)[1] for n in range(N)]
    for c, k in enumerate(('rhs', 'rho')):
        err, floor = G.rel_l2(stack.grad[:, c].cpu(), _stack(ref, k)), G.rel_l2(_stack(low, k), _stack(ref, k))
        print('residual 19 x 70 mask %d d%s: rel-L2 %.3g, fp32 floor %.3g' % (mask, k, err, floor))
        assert err <= 4.0 * floor, (k, err, floor)
    # only pred requires grad: the stack gets none
    pred2 = pred.detach().clone().requires_grad_(True)
    autograd.variable_density_residual(pred2, stack.detach(), d_dx).sum().backward()
    assert pred2.grad is not None


def test_c_abi_refusals(ops):
    import ctypes
    H, W = 4, 5
    u, lam0, rho, rhs, du, edges, dx, coef = _case(H, W)
    N = u.shape[0]
    d_u, d_lam, d_rho, d_rhs, d_dx, d_coef = _dev(u), _dev(lam0 * G.unknown_mask(H, W, 0).numpy()), _dev(rho), _dev(rhs), _dev(dx), _dev(coef)
    p, ci, call = ops._p, ctypes.c_int, ops.handle().call
    y = torch.empty_like(d_u)
    for bad in (16, -1):
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_coef_grad', ci(N), ci(H), ci(W), ci(bad), p(d_rho), p(d_dx), p(d_u), p(d_lam), p(None), p(None), p(None), p(None), p(y))
        with pytest.raises(RuntimeError, match='neumann_mask'):
            call('pcnn_varcoef_bc_pi_loss_bwd_inputs', ci(N), ci(H), ci(W), p(d_u), p(d_rho), p(d_rhs), p(d_dx), p(d_coef), p(y), p(None), ci(bad))
        with pytest.raises(ValueError, match='neumann_mask'):
            ops.varcoef_edge_grad(d_lam, d_rho, d_dx, bad)
    with pytest.raises(RuntimeError, match='unsupported'):
        call('pcnn_varcoef_bc_coef_grad', ci(N), ci(2), ci(10), ci(0), p(d_rho), p(d_dx), p(d_u), p(d_lam), p(None), p(None), p(None), p(None), p(y))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_coef_grad', ci(N), ci(H), ci(W), ci(0), p(d_rho), p(d_dx), p(d_u), p(d_lam), p(None), p(None), p(None), p(None), p(d_u))
    with pytest.raises(RuntimeError, match='alias'):
        call('pcnn_varcoef_bc_pi_loss_bwd_inputs', ci(N), ci(H), ci(W), p(d_u), p(d_rho), p(d_rhs), p(d_dx), p(d_coef), p(d_rhs), p(None), ci(0))
    with pytest.raises(ValueError, match='contiguous CUDA float32'):
        ops.varcoef_coef_grad(d_lam, d_u, d_rho, d_dx, 1, {'left': torch.zeros(N, W + 1, device='cuda')})


def test_ten_descent_steps_on_the_density_reduce_the_misfit():
    """Plain gradient descent on rho from rho = 2 towards the density that made u_true (tests/varcoef_grad_twin.gd_problem), with the step size the
    twin needs: ||u(rho) - u_true||^2 falls at every step."""
    from poisson_cnn_amd import autograd
    rho_true, rhs, edges, u_true = G.gd_problem()
    H, W = G.GD_SHAPE
    d_rhs, d_true = _dev(rhs.numpy()[None]), _dev(u_true.numpy()[None])
    d_edges = {k: _dev(v.numpy()[None]) for k, v in edges.items()}
    dx = torch.full((1,), G.GD_DX, device='cuda')
    rho = torch.full((1, H, W), 2.0, device='cuda')
    hist = []
    for _ in range(G.GD_STEPS + 1):
        rho = rho.detach().requires_grad_(True)
        obj = (autograd.variable_density_solve(rho, d_rhs, d_edges, dx)[:, 0] - d_true).double().square().sum()
        hist.append(float(obj.detach()))
        obj.backward()
        rho = rho - G.GD_STEP * rho.grad
    print('descent on rho, 17 x 65: objective', ' '.join('%.4g' % v for v in hist))
    assert all(b < a for a, b in zip(hist, hist[1:])), hist
