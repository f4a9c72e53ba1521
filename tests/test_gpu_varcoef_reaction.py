"""The variable-density solve with a reaction term, div((1/rho) grad u) - c u = f (the *_reaction entry points of poisson_cnn_amd/csrc/varcoef.hip,
DESIGN.md section 26), against the fp64 twin of tests/varcoef_reaction_twin.py (whose own properties tests/test_varcoef_reaction_reference.py checks
without a GPU).

Shapes against the 16 x 64 operator tile: (5, 4) is less than one tile with 3 x 2 interior points, (21, 70) passes one tile on both axes with neither
count a multiple of it, (35, 131) passes two tiles along W.  Batch 3: density ratios 1, 10, 100, one spacing per sample from [5e-3, 5e-2], and c per
node = m s / (rho dx^2) with s smooth in [0.5, 1.5] and m = 0.1, 10, 1e3 - negligible against the operator's diagonal in one sample, comparable in one,
dominant in one.  Masks 0 (all Dirichlet), 5, 10 and 15 (all Neumann: nonsingular here).

Bounds, those of tests/test_gpu_varcoef.py: 1e-12 rel-L2 for the operator and 1e-12 for p.q - both sides are fp64 and a point's sum has one more
fused term; 2e-7 rel-L2 for a solution - the output is fp32."""
import functools

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_reaction_twin as R
from tests import varcoef_twin as T

pytestmark = pytest.mark.gpu
EDGES = B.EDGES
CHECK = 8
N = 3
SHAPES = [(5, 4), (21, 70), (35, 131)]
MASKS = [0, 5, 10, 15]
RATIOS = (1.0, 10.0, 100.0)
MAGNITUDES = (0.1, 10.0, 1e3)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def problem(H, W, ratios=RATIOS, magnitudes=MAGNITUDES):
    """float32-representable inputs, one sample per density ratio; read, never written."""
    n = len(ratios)
    rng = np.random.default_rng(1000 * H + W)
    rho = f32(np.stack([T.smooth_density(rng, H, W, 1.0, r) if r > 1.0 else np.ones((H, W)) for r in ratios]))
    f = f32(rng.uniform(-1, 1, (n, H, W)) + 1.5)                    # a mean far from 0: so is the solution's, which the all-Neumann case must keep
    e = {k: f32(rng.uniform(-1, 1, (n, W if k in ('left', 'right') else H))) for k in EDGES}
    dx = f32(rng.uniform(5e-3, 5e-2, n))
    c = f32(np.stack([m * T.smooth_density(rng, H, W, 0.5, 1.5) / (rho[k] * dx[k] ** 2) for k, m in enumerate(magnitudes)]))
    return rho, c, f, e, dx


@functools.lru_cache(maxsize=None)
def twin(H, W, mask):
    """Per sample: the direct solution (n,H,W) and the twin recurrence's iteration counts at tol 1e-10."""
    rho, c, f, e, dx = problem(H, W)
    its = []
    for n in range(rho.shape[0]):
        AC, b = R.assemble(rho[n], c[n], dx[n], mask, {k: v[n] for k, v in e.items()}, f[n])
        _, it, res = R.pcg(AC, b, rho[n], c[n], dx[n], mask, tol=1e-10, max_iterations=500)
        assert res <= 1e-10, (H, W, mask, n, it, res)                          # the data are such that the twin converges within 500
        its.append(it)
    return R.solve_batch(rho, c, f, e, dx, mask), its


def solve(rho, c, f, e, dx, mask, **kw):
    from poisson_cnn_amd import dataset as D
    extra = {} if c is None else {'reaction': c if isinstance(c, torch.Tensor) else dev(c)}
    return D.variable_density_poisson_solve(dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx), return_info=True, boundary_types=B.types(mask),
                                            **extra, **kw)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_operator_matches_the_sparse_matrix(H, W, mask):
    from poisson_cnn_amd.dataset import _kernels as K
    rho, c, _, _, dx = problem(H, W)
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    mh, mw = i1 - i0 + 1, j1 - j0 + 1
    p = np.random.default_rng(H + W + mask).standard_normal((N, mh, mw))
    w = B.weights(H, W, mask)
    ref = np.stack([(R.assemble(rho[n], c[n], dx[n], mask)[0] @ p[n].ravel()).reshape(mh, mw) for n in range(N)])
    args = (dev(rho), dev(dx), dev(p, torch.float64))
    q, pq = K.varcoef_apply(*args, neumann=B.flags(mask), reaction=dev(c))
    q2, pq2 = K.varcoef_apply(*args, neumann=B.flags(mask), reaction=dev(c))
    assert tuple(q.shape) == (N, mh, mw)
    ref_pq = np.einsum('ij,nij,nij->n', w, p, ref)
    err, err_pq = rel(q.cpu().numpy(), ref), np.abs(pq.cpu().numpy() - ref_pq).max() / np.abs(ref_pq).max()
    print('%dx%d mask %d: operator rel-L2 %.3e, weighted p.q rel %.3e' % (H, W, mask, err, err_pq))
    assert err <= 1e-12
    assert err_pq <= 1e-12
    assert torch.equal(q, q2) and torch.equal(pq, pq2)
    if mask == 0:                                                                 # neumann = None is the family's mask 0
        q0, pq0 = K.varcoef_apply(*args, reaction=dev(c))
        assert torch.equal(q, q0) and torch.equal(pq, pq0)
    plain = K.varcoef_apply(*args, neumann=B.flags(mask))[0]                      # the term is there: the dominant sample differs by far more than rounding
    assert rel(q[2].cpu().numpy(), plain[2].cpu().numpy()) > 1.0


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_solve_matches_the_direct_sparse_solve(H, W, mask):
    rho, c, f, e, dx = problem(H, W)
    ref, its = twin(H, W, mask)
    soln, info = solve(rho, c, f, e, dx, mask, tol=1e-10, max_iterations=500)
    assert tuple(soln.shape) == (N, 1, H, W) and soln.dtype == torch.float32
    s = soln[:, 0].cpu().numpy().astype(np.float64)
    errs = [rel(s[n], ref[n]) for n in range(N)]
    print('%dx%d mask %d: solve rel-L2 %r, iterations %r (twin %r)' % (H, W, mask, errs, info['iterations'].tolist(), its))
    assert max(errs) <= 2e-7
    assert info['converged'].all() and (info['relative_residual'] <= 1e-10).all()
    for n, it in enumerate(its):
        assert info['iterations'][n] % CHECK == 0
        assert info['iterations'][n] <= it + CHECK, (n, it, info['iterations'][n])
    if mask:
        assert not info['compatibility_defect'].any() and not info['rhs_shift'].any()
    if mask == 15:        # no mean was removed: the solution's weighted mean is far from 0 - at least 1e-2 of its rms, 5e4 times the bound above
        w = B.weights(H, W, 15)
        for n in range(N):
            assert abs((w * ref[n]).sum() / w.sum()) >= 1e-2 * np.sqrt((w * ref[n] ** 2).sum() / w.sum()), n
            assert abs((w * s[n]).sum() - (w * ref[n]).sum()) <= 2e-7 * w.sum() * np.abs(ref[n]).max()


def test_none_is_the_call_without_the_keyword_and_zeros_agree_with_it():
    from poisson_cnn_amd import dataset as D
    H, W = 21, 70
    rho, _, f, e, dx = problem(H, W)
    for mask in (0, 5):
        a = (dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx))
        kw = dict(return_info=True, boundary_types=B.types(mask))
        base, info = D.variable_density_poisson_solve(*a, **kw)
        none, info_none = D.variable_density_poisson_solve(*a, reaction=None, **kw)
        assert torch.equal(base, none) and all(np.array_equal(info[k], info_none[k]) for k in info)
        zero, info_zero = D.variable_density_poisson_solve(*a, reaction=np.zeros((N, H, W), dtype=np.float32), **kw)
        errs = [rel(zero[n, 0].cpu().numpy(), base[n, 0].cpu().numpy()) for n in range(N)]
        print('mask %d: reaction of zeros against the plain solve, rel-L2 %r' % (mask, errs))
        assert max(errs) <= 2e-7 and info_zero['converged'].all()                  # (not bits: the preconditioner's scaling differs)


def test_one_number_per_sample_is_the_broadcast_field_bit_for_bit():
    H, W = 21, 70
    rho, c, f, e, dx = problem(H, W)
    per = f32(c.reshape(N, -1).mean(axis=1))
    for mask in (0, 15):
        field, info = solve(rho, np.broadcast_to(per[:, None, None], (N, H, W)).copy(), f, e, dx, mask)
        for form in (per, per[:, None], dev(per)):
            got, info_got = solve(rho, form, f, e, dx, mask)
            assert torch.equal(field, got) and np.array_equal(info['iterations'], info_got['iterations'])


def test_a_sample_does_not_depend_on_its_batch_two_runs_agree_and_a_converged_one_is_frozen():
    H, W = 45, 70
    rho, c, f, e, dx = (a.copy() if isinstance(a, np.ndarray) else {k: v.copy() for k, v in a.items()} for a in problem(H, W, (100.0, 1.0), (10.0, 10.0)))
    c[1] = f32(c[1].mean())                                         # rho = 1 and a constant c: the preconditioner is exact, converged at the first look
    for mask in (0, 10):
        one = lambda n: (rho[n:n + 1], c[n:n + 1], f[n:n + 1], {k: v[n:n + 1] for k, v in e.items()}, dx[n:n + 1])
        both, info = solve(rho, c, f, e, dx, mask)
        again, info_again = solve(rho, c, f, e, dx, mask)
        hard, info_hard = solve(*one(0), mask)
        easy, info_easy = solve(*one(1), mask)
        print(mask, info, info_hard, info_easy)
        assert torch.equal(both, again) and np.array_equal(info['relative_residual'], info_again['relative_residual'])
        assert info['iterations'][0] > CHECK and info_easy['iterations'][0] == CHECK      # the easy sample sat frozen while the hard one went on
        assert torch.equal(both[0], hard[0]) and info['iterations'][0] == info_hard['iterations'][0]
        assert torch.equal(both[1], easy[0]) and info['iterations'][1] == CHECK           # its own 8 iterations, bit for bit


def fill_free_blocks(words, value):
    """Leaves `value` in the allocator's free blocks of `words` doubles (four are filled and freed together, so the block of an earlier solve is
    among them) -> what a fresh torch.empty of that size then holds."""
    held = [torch.full((words,), value, dtype=torch.float64, device='cuda') for _ in range(4)]
    torch.cuda.synchronize()
    del held
    probe = torch.empty((words,), dtype=torch.float64, device='cuda')
    seen = probe.clone()
    del probe
    return seen


def test_result_does_not_depend_on_what_the_workspace_held():
    from ctypes import c_int
    from poisson_cnn_amd import _lib
    H, W = 21, 70
    rho, c, f, e, dx = problem(H, W)
    for mask in (0, 15):
        words = (int(_lib.load().pcnn_varcoef_bc_pcg_workspace_reaction(c_int(N), c_int(H), c_int(W), c_int(mask))) + 7) // 8
        guess = torch.tensor(twin(H, W, mask)[0][:, None], dtype=torch.float64)
        runs = {}
        for value in (0.0, float('nan')):
            for name, kw in (('cold', {}), ('at the solution', {'initial_guesses': guess})):
                seen = fill_free_blocks(words, value)
                assert bool(torch.isnan(seen).all()) == (value != 0.0)            # the allocator does hand the filled block back
                runs[name, value != 0.0] = solve(rho, c, f, e, dx, mask, **kw)
        for name in ('cold', 'at the solution'):
            (clean, info), (dirty, info_dirty) = runs[name, False], runs[name, True]
            assert torch.isfinite(dirty).all() and np.isfinite(info_dirty['relative_residual']).all()
            assert torch.equal(clean, dirty)
            assert np.array_equal(info['iterations'], info_dirty['iterations']) and info_dirty['converged'].all()
            assert np.array_equal(info['relative_residual'], info_dirty['relative_residual'])
        assert (runs['at the solution', False][1]['iterations'] == CHECK).all()


def test_device_refusals():
    H, W = 21, 70
    rho, c, f, e, dx = problem(H, W)
    for bad in (-1.0, float('nan'), float('inf')):
        field = c.copy()
        field[1, 7, 9] = bad
        with pytest.raises(ValueError, match='reaction'):
            solve(rho, dev(field), f, e, dx, 5)                                    # found by the setup kernel's minimum: a device tensor
    ring = c.copy()
    ring[:, 0, :] = np.nan                                                         # a Dirichlet edge's nodes are not unknowns: never read
    assert solve(rho, dev(ring), f, e, dx, 0)[1]['converged'].all()
    with pytest.raises(ValueError, match='scaled'):
        solve(rho, dev(c), f, e, dx, 0, preconditioner='scaled')
    zero = c.copy()
    zero[1] = 0.0
    with pytest.raises(ValueError, match='singular'):
        solve(rho, dev(zero), f, e, dx, 15)
    assert solve(rho, dev(zero), f, e, dx, 10)[1]['converged'].all()               # with a Dirichlet edge that sample is fine


def test_generator_yields_the_reaction_channel_and_none_is_the_generator_as_it_was():
    """reaction_range = None against tests/golden/varcoef_generator_parent.npz: the batch the generator drew at the commit before it knew the
    keyword (tools/record_varcoef_generator_golden.py), bit for bit."""
    import os
    import sys
    from poisson_cnn_amd import dataset as D
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import record_varcoef_generator_golden as G
    finally:
        sys.path.pop(0)
    golden = np.load(G.GOLDEN)
    kw = G.KW
    for case, types in G.CASES.items():
        mask = 15 if types else 0
        now = G.run(case, reaction_range=None)
        for k in G.NAMES:
            assert now[k].dtype == golden['%s/%s' % (case, k)].dtype and np.array_equal(now[k], golden['%s/%s' % (case, k)]), (case, k)
        (inp, soln), (inp0, soln0) = (D.variable_density_dataset_generator(boundary_types=types, **extra, **kw)[0] for extra in ({'reaction_range': (0.5, 50.0)}, {}))
        stack, left, top, right, bottom, dx = inp
        assert tuple(stack.shape) == (2, 3, 33, 47) and tuple(inp0[0].shape) == (2, 2, 33, 47) and tuple(soln.shape) == (2, 1, 33, 47)
        cfield = stack[:, 2]
        assert float(cfield.min()) >= 0.5 and float(cfield.max()) <= 50.0 and float(cfield.max()) > 2 * float(cfield.min())
        assert torch.equal(stack[:, 1], inp0[0][:, 1]) and all(torch.equal(a, b) for a, b in zip(inp[1:], inp0[1:]))   # drawn last: the other draws did not move
        if mask == 0:
            assert torch.equal(stack[:, 0], inp0[0][:, 0])
        host = lambda t: t.cpu().numpy().astype(np.float64)
        edges = {'left': host(left[:, 0]), 'right': host(right[:, 0]), 'bottom': host(bottom[:, 0]), 'top': host(top[:, 0])}
        w = B.weights(33, 47, mask).ravel()
        for n in range(2):
            rho, c, f, h = host(stack[n, 1]), host(cfield[n]), host(stack[n, 0]), float(host(dx[n, 0]))
            AC, b = R.assemble(rho, c, h, mask, {k: v[n] for k, v in edges.items()}, f)
            res = lambda u: np.sqrt((w * (b - AC @ R.on_unknowns(u, mask).ravel()) ** 2).sum() / (w * b * b).sum())
            floor = res(f32(R.solve(rho, c, f, {k: v[n] for k, v in edges.items()}, h, mask)))
            got = res(host(soln[n, 0]))
            print('mask %d sample %d: relative residual of the yielded solution %.3e, of the fp32-rounded direct solution %.3e' % (mask, n, got, floor))
            # the fp32 rounding of u limits the figure: the fp32-rounded fp64 direct solution is the floor, measured here per sample, and the bound is 4 floors
            # Measured on an MI355X: yielded 1.137e-07 / 1.549e-07 (mask 0) and 5.065e-07 / 1.310e-06 (mask 15), the floors the same figures to
            # the digits printed - all below the 2e-6 that fp32 allows here.
            assert got <= 4.0 * floor and got <= 2e-6
