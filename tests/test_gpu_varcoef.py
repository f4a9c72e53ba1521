"""The variable-density Poisson operator and its DST-preconditioned conjugate-gradient solve (poisson_cnn_amd/csrc/varcoef.hip) and the generator built on
them, against the fp64 twin of tests/varcoef_twin.py (whose own properties tests/test_varcoef_reference.py checks without a GPU).

Bounds: 1e-12 rel-L2 for the operator - both sides are fp64 and a point's sum has five terms; 2e-7 rel-L2 for a solution - the bound
tests/test_gpu_dataset.py uses for the mixed solver's fp32 output of an fp64 solve."""
import functools

import numpy as np
import pytest
import torch

from tests import varcoef_twin as T

pytestmark = pytest.mark.gpu
EDGES = ('left', 'right', 'bottom', 'top')
CHECK = 8


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def problem(seed, N, H, W, ratios):
    """float32-representable inputs of N samples, a density ratio per sample; read, never written."""
    rng = np.random.default_rng(seed)
    rho = f32(np.stack([T.smooth_density(rng, H, W, 1.0, r) for r in ratios]))
    f = f32(rng.uniform(-1, 1, (N, H, W)))
    b = {k: f32(rng.uniform(-1, 1, (N, W if k in ('left', 'right') else H))) for k in EDGES}
    dx = f32(rng.uniform(5e-3, 5e-2, N))
    return rho, f, b, dx


@functools.lru_cache(maxsize=None)
def twin_solution(seed, N, H, W, ratios):
    rho, f, b, dx = problem(seed, N, H, W, ratios)
    return T.solve_batch(rho, f, b, dx)


@functools.lru_cache(maxsize=None)
def twin_iterations(seed, N, H, W, ratios):
    rho, f, b, dx = problem(seed, N, H, W, ratios)
    return [T.pcg(T.assemble(rho[n], dx[n]), T.right_hand_side(rho[n], f[n], {k: v[n] for k, v in b.items()}, dx[n]), (H - 2, W - 2), tol=1e-10)[1] for n in range(N)]


def solve(rho, f, b, dx, **kw):
    from poisson_cnn_amd import dataset as D
    return D.variable_density_poisson_solve(dev(rho), dev(f), {k: dev(v) for k, v in b.items()}, dev(dx), return_info=True, **kw)


@pytest.mark.parametrize('H,W', [(19, 23), (64, 64), (65, 130)])
def test_operator_matches_the_sparse_matrix(H, W):
    """19x23: one partial tile; 64x64: 62 interior columns, four row tiles; 65x130: interior 63 x 128 = whole column tiles, a partial row tile."""
    from poisson_cnn_amd.dataset import _kernels as K
    N = 3
    rho, _, _, dx = problem(H * W, N, H, W, (1.0, 10.0, 100.0))
    rng = np.random.default_rng(H + W)
    p = rng.standard_normal((N, H - 2, W - 2))
    ref = np.stack([(T.assemble(rho[n], dx[n]) @ p[n].ravel()).reshape(H - 2, W - 2) for n in range(N)])
    q, pq = K.varcoef_apply(dev(rho), dev(dx), dev(p, torch.float64))
    q2, pq2 = K.varcoef_apply(dev(rho), dev(dx), dev(p, torch.float64))
    err = rel(q.cpu().numpy(), ref)
    ref_pq = np.einsum('nij,nij->n', p, ref)
    err_pq = np.abs(pq.cpu().numpy() - ref_pq).max() / np.abs(ref_pq).max()
    print('operator rel-L2 %.3e, p.q rel %.3e' % (err, err_pq))
    assert err <= 1e-12
    assert err_pq <= 1e-12
    assert torch.equal(q, q2) and torch.equal(pq, pq2)


@pytest.mark.parametrize('H,W', [(33, 47), (97, 65)])
def test_solve_matches_the_direct_sparse_solve(H, W):
    key = (H + W, 3, H, W, (10.0, 10.0, 10.0))
    rho, f, b, dx = problem(*key)
    ref = twin_solution(*key)
    soln, info = solve(rho, f, b, dx, tol=1e-10)
    assert tuple(soln.shape) == (3, 1, H, W) and soln.dtype == torch.float32
    s = soln[:, 0].cpu().numpy().astype(np.float64)
    errs = [rel(s[n], ref[n]) for n in range(3)]
    print('solve rel-L2', errs, info)
    assert max(errs) <= 2e-7
    assert np.array_equal(s[:, 0, :], b['left']) and np.array_equal(s[:, -1, :], b['right'])
    assert np.array_equal(s[:, 1:-1, 0], b['bottom'][:, 1:-1]) and np.array_equal(s[:, 1:-1, -1], b['top'][:, 1:-1])
    assert info['converged'].all() and (info['relative_residual'] <= 1e-10).all()
    # no more iterations than the twin's recurrence, at the granularity the host looks at the flags, plus one look of slack
    for n, it in enumerate(twin_iterations(*key)):
        assert info['iterations'][n] % CHECK == 0
        assert info['iterations'][n] <= -(-it // CHECK) * CHECK + CHECK, (n, it, info['iterations'][n])


def test_unit_density_is_the_dst_solve_in_one_look():
    from poisson_cnn_amd import dataset as D
    _, f, b, dx = problem(3, 2, 41, 38, (1.0, 1.0))
    soln, info = solve(np.ones_like(f), f, b, dx)
    ref = D.multigrid_poisson_solve(dev(f), {k: dev(v) for k, v in b.items()}, dev(dx))
    err = rel(soln.cpu().numpy(), ref.cpu().numpy())
    print('rho = 1 against the DST solve: rel-L2 %.3e' % err, info)
    assert err <= 2e-7
    assert (info['iterations'] == CHECK).all() and info['converged'].all()        # the preconditioner is exact: converged at the first look


def test_a_sample_does_not_depend_on_its_batch_and_a_converged_one_is_frozen():
    H, W = 45, 70
    rho, f, b, dx = problem(4, 2, H, W, (100.0, 1.0))
    rho = rho.copy()
    rho[1] = 1.0
    one = lambda n: (rho[n:n + 1], f[n:n + 1], {k: v[n:n + 1] for k, v in b.items()}, dx[n:n + 1])
    both, info = solve(rho, f, b, dx)
    hard, info_hard = solve(*one(0))
    easy, info_easy = solve(*one(1))
    print(info, info_hard, info_easy)
    assert info['iterations'][0] > CHECK and info_easy['iterations'][0] == CHECK      # the easy sample sat frozen while the hard one went on
    assert torch.equal(both[0], hard[0]) and info['iterations'][0] == info_hard['iterations'][0]
    assert torch.equal(both[1], easy[0])                                              # ... and its solution is the one of its own 8 iterations, bit for bit
    assert info['iterations'][1] == CHECK


def test_initial_guess_at_the_solution_needs_one_look():
    key = (33 + 47, 3, 33, 47, (10.0, 10.0, 10.0))
    rho, f, b, dx = problem(*key)
    ref = twin_solution(*key)
    soln, info = solve(rho, f, b, dx, initial_guesses=torch.tensor(ref[:, None], dtype=torch.float64))
    assert (info['iterations'] == CHECK).all() and info['converged'].all()
    assert max(rel(soln[n, 0].cpu().numpy(), ref[n]) for n in range(3)) <= 2e-7


def fill_free_blocks(N, H, W, value):
    """Leaves `value` in the allocator's free blocks of the solve's workspace size: four such tensors are filled and freed together, so the block
    of an earlier solve is among them.  Returns what a fresh torch.empty of that size then holds."""
    from ctypes import c_int
    from poisson_cnn_amd import _lib
    words = (int(_lib.load().pcnn_varcoef_pcg_workspace(c_int(N), c_int(H), c_int(W))) + 7) // 8
    held = [torch.full((words,), value, dtype=torch.float64, device='cuda') for _ in range(4)]
    torch.cuda.synchronize()
    del held
    probe = torch.empty((words,), dtype=torch.float64, device='cuda')
    seen = probe.clone()
    del probe
    return seen


def test_result_does_not_depend_on_what_the_workspace_held():
    """The workspace is not cleared.  Before the first direction p is unwritten memory, and 0 * NaN is NaN: a solve into blocks that held NaN must
    give the bits of a solve into blocks that held zeros - from a zero start, and from a start at the solution (flagged at setup, x += 0 * p)."""
    key = (33 + 47, 3, 33, 47, (10.0, 10.0, 10.0))
    rho, f, b, dx = problem(*key)
    guess = torch.tensor(twin_solution(*key)[:, None], dtype=torch.float64)
    runs = {}
    for value in (0.0, float('nan')):
        for name, kw in (('cold', {}), ('at the solution', {'initial_guesses': guess})):
            seen = fill_free_blocks(3, 33, 47, value)
            assert bool(torch.isnan(seen).all()) == (value != 0.0)              # the allocator does hand the filled block back
            runs[name, value != 0.0] = solve(rho, f, b, dx, **kw)
    for name in ('cold', 'at the solution'):
        (clean, info), (dirty, info_dirty) = runs[name, False], runs[name, True]
        assert torch.isfinite(dirty).all() and np.isfinite(info_dirty['relative_residual']).all()
        assert torch.equal(clean, dirty)
        assert np.array_equal(info['iterations'], info_dirty['iterations']) and info_dirty['converged'].all()
        assert np.array_equal(info['relative_residual'], info_dirty['relative_residual'])


def test_running_out_of_iterations_warns_and_returns():
    H = W = 49
    rng = np.random.default_rng(7)
    rho = f32(T.smooth_density(rng, H, W, 1.0, 1e4))[None]
    f = f32(rng.uniform(-1, 1, (1, H, W)))
    b = {k: f32(rng.uniform(-1, 1, (1, H))) for k in EDGES}
    dx = f32([0.02])
    _, it, twin_rel = T.pcg(T.assemble(rho[0], dx[0]), T.right_hand_side(rho[0], f[0], {k: v[0] for k, v in b.items()}, dx[0]), (H - 2, W - 2), max_iterations=8)
    assert it == 8 and twin_rel < 1.0                                                 # the twin is not there either (0.107)
    with pytest.warns(RuntimeWarning, match='not converged'):
        soln, info = solve(rho, f, b, dx, max_iterations=8)
    print(info, twin_rel)
    assert not info['converged'][0] and info['iterations'][0] == 8
    assert np.isfinite(info['relative_residual'][0]) and info['relative_residual'][0] < 1.0
    assert abs(info['relative_residual'][0] - twin_rel) <= 1e-6 * twin_rel            # the same eight steps as the twin's recurrence
    assert torch.isfinite(soln).all()


def test_refusals():
    rho, f, b, dx = problem(5, 2, 20, 21, (2.0, 3.0))
    bad = rho.copy()
    bad[1, 7, 9] = 0.0
    with pytest.raises(ValueError, match='positive'):
        solve(bad, f, b, dx)                                                          # found by the setup kernel's minimum: rho is a device tensor here
    bad[1, 7, 9] = np.nan
    with pytest.raises(ValueError, match='positive'):
        solve(bad, f, b, dx)                                                          # a NaN counts as -inf in that minimum
    with pytest.raises(NotImplementedError):
        solve(rho, f, b, dx, dy=2 * dx)


def test_generator_batches():
    from poisson_cnn_amd import dataset as D
    kw = dict(batch_size=2, batches_per_epoch=2, random_output_shape_range=((33, 40), (41, 48)), density_range=(1.0, 10.0), rhs_smoothness_range=(4, 7),
              density_smoothness_range=(3, 6), boundaries='random', seed=9)
    gen, again = D.variable_density_dataset_generator(**kw), D.variable_density_dataset_generator(**kw)
    assert len(gen) == 2
    for _ in range(2):
        inp, soln = gen[0]
        inp2, soln2 = again[0]
        frho, left, top, right, bottom, dx = inp
        N, _, H, W = frho.shape
        assert N == 2 and 33 <= H <= 40 and 41 <= W <= 48
        assert tuple(soln.shape) == (2, 1, H, W) and tuple(dx.shape) == (2, 1)
        assert tuple(left.shape) == tuple(right.shape) == (2, 1, W) and tuple(top.shape) == tuple(bottom.shape) == (2, 1, H)
        rho = frho[:, 1].cpu().numpy().astype(np.float64)
        assert rho.min() >= 1.0 and rho.max() <= 10.0 and rho.max() / rho.min() > 2.0
        assert gen.last_info['converged'].all()
        edges = {'left': left, 'right': right, 'bottom': bottom, 'top': top}
        ref = T.solve_batch(rho, frho[:, 0].cpu().numpy().astype(np.float64), {k: v[:, 0].cpu().numpy().astype(np.float64) for k, v in edges.items()},
                            dx[:, 0].cpu().numpy().astype(np.float64))
        errs = [rel(soln[n, 0].cpu().numpy(), ref[n]) for n in range(2)]
        print('generator batch rel-L2', errs)
        assert max(errs) <= 2e-7
        assert torch.equal(soln, soln2) and all(torch.equal(a, c) for a, c in zip(inp, inp2))
    soln, frho = D.variable_density_dataset_generator(batch_size=1, output_shape=(20, 24), boundaries='zero', return_keras_style=False, seed=1)[0]
    assert tuple(soln.shape) == (1, 1, 20, 24) and tuple(frho.shape) == (1, 2, 20, 24)
    assert float(soln[:, :, 0].abs().max()) == 0.0 and float(soln[:, :, :, -1].abs().max()) == 0.0
