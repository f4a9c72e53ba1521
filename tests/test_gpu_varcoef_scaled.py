"""The diagonally scaled preconditioner of the variable-density solve (preconditioner='scaled': the *_scaled entry points of
poisson_cnn_amd/csrc/varcoef.hip) and the generator's smooth density profile, against the fp64 twins of
tests/varcoef_scaled_twin.py, whose own properties tests/test_varcoef_scaled_reference.py checks without a GPU.

Fixture: the smooth density of ratio 1000 (sample 0: smooth_density(default_rng(0), ..); samples 1 and 2 further draws), batch 3, at 33 x 47 and
45 x 70 (neither a multiple of the 16 x 64 tile) and 97 x 65; masks 0, 1 (left Neumann) and 15; check_every = 8.
Bounds are those of tests/test_gpu_varcoef.py: 2e-7 rel-L2 for an fp32 solution of an fp64 solve, 1e-10 for the relative residual.  Iterations:
at most the twin's scaled count rounded up to a look, plus one look; and at most half of what preconditioner='dst' - the code every solve ran
before - takes in the same test."""
import functools
from ctypes import c_double, c_int, c_size_t

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_scaled_twin as S
from tests import varcoef_twin as T

pytestmark = pytest.mark.gpu
EDGES = B.EDGES
CHECK = 8
N = 3
RATIO = 1000.0
SHAPES = [(33, 47), (45, 70), (97, 65)]
MASKS = [0, 1, 15]


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def sample(e, n):
    return {k: v[n] for k, v in e.items()}


@functools.lru_cache(maxsize=None)
def problem(H, W):
    """float32-representable inputs of the N samples; read, never written."""
    return S.smooth_fixture(H, W, RATIO, N)


@functools.lru_cache(maxsize=None)
def twin(H, W, mask):
    """Per sample: (the direct sparse solution, the twin's scaled iteration count)."""
    rho, f, e, dx = problem(H, W)
    out = []
    for n in range(N):
        A, b = B.assemble(rho[n], dx[n], mask, sample(e, n), f[n])
        out.append((B.solve(rho[n], f[n], sample(e, n), dx[n], mask), S.pcg(A, b, H, W, mask, dx[n], tol=1e-10)[1]))
    return out


def solve(rho, f, e, dx, mask, **kw):
    """mask 0 goes through the all-Dirichlet entry points (no boundary_types), any other through the *_bc_* ones."""
    from poisson_cnn_amd import dataset as D
    if mask:
        kw['boundary_types'] = B.types(mask)
    return D.variable_density_poisson_solve(dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx), return_info=True, check_every=CHECK, **kw)


def one(p, n):
    rho, f, e, dx = p
    return rho[n:n + 1], f[n:n + 1], {k: v[n:n + 1] for k, v in e.items()}, dx[n:n + 1]


# ----------------------------------------------------------------------------- 1. solution and iteration counts
@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('mask', MASKS)
def test_scaled_solve_matches_the_direct_solve_in_at_most_half_the_iterations(mask, H, W):
    rho, f, e, dx = problem(H, W)
    ref = twin(H, W, mask)
    soln, info = solve(rho, f, e, dx, mask, tol=1e-10, preconditioner='scaled')
    plain, info_plain = solve(rho, f, e, dx, mask, tol=1e-10, preconditioner='dst')
    assert tuple(soln.shape) == (N, 1, H, W) and soln.dtype == torch.float32
    s = soln[:, 0].cpu().numpy().astype(np.float64)
    errs = [rel(s[n], ref[n][0]) for n in range(N)]
    errs_plain = [rel(plain[n, 0].cpu().numpy(), ref[n][0]) for n in range(N)]
    print('mask %d %dx%d: rel-L2 scaled %s, dst %s; iterations twin (scaled) %s, scaled %s, dst %s; residual %s'
          % (mask, H, W, errs, errs_plain, [r[1] for r in ref], info['iterations'].tolist(), info_plain['iterations'].tolist(), info['relative_residual'].tolist()))
    assert max(errs) <= 2e-7 and max(errs_plain) <= 2e-7
    assert info['converged'].all() and (info['relative_residual'] <= 1e-10).all() and info_plain['converged'].all()
    assert set(info) == set(info_plain)
    for n in range(N):
        assert info['iterations'][n] % CHECK == 0
        assert info['iterations'][n] <= -(-ref[n][1] // CHECK) * CHECK + CHECK, (n, ref[n][1], info['iterations'][n])
        assert 2 * info['iterations'][n] <= info_plain['iterations'][n], (n, info['iterations'][n], info_plain['iterations'][n])
    nl, nr, nb, nt = B.flags(mask)                                      # a Dirichlet edge holds its values, rows 0 / H-1 first
    if not nl:
        assert np.array_equal(s[:, 0, :], e['left'])
    if not nr:
        assert np.array_equal(s[:, -1, :], e['right'])
    if not nb:
        assert np.array_equal(s[:, 1:-1, 0], e['bottom'][:, 1:-1])
    if not nt:
        assert np.array_equal(s[:, 1:-1, -1], e['top'][:, 1:-1])


# ----------------------------------------------------------------------------- 2. the default is the code as it was
@pytest.mark.parametrize('mask', [0, 5])
def test_dst_is_bit_equal_to_a_call_without_the_keyword(mask):
    from poisson_cnn_amd import dataset as D
    rho, f, e, dx = problem(45, 70)
    kw = {'boundary_types': B.types(mask)} if mask else {}
    d = lambda: (dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx))
    today, info_today = D.variable_density_poisson_solve(*d(), return_info=True, **kw)
    named, info_named = D.variable_density_poisson_solve(*d(), return_info=True, preconditioner='dst', **kw)
    assert torch.equal(today, named) and set(info_today) == set(info_named)
    for k in info_today:
        assert np.array_equal(info_today[k], info_named[k]), k
    assert info_today['iterations'].max() > CHECK
    assert torch.equal(D.compressible_poisson_solve(*d(), preconditioner='dst'), D.compressible_poisson_solve(*d()))
    if not mask:
        assert torch.equal(today, D.compressible_poisson_solve(*d()))
        scaled = D.variable_density_poisson_solve(*d(), preconditioner='scaled')
        assert torch.equal(D.compressible_poisson_solve(*d(), preconditioner='scaled'), scaled) and not torch.equal(scaled, today)


# ----------------------------------------------------------------------------- 3. independence of the batch, frozen samples, determinism
@pytest.mark.parametrize('mask', MASKS)
def test_a_sample_does_not_depend_on_its_batch_and_a_converged_one_stays_frozen(mask):
    """Sample 1 gets rho = 1: s = 1 there, the preconditioner is exact and the sample is flagged at the first look, while its neighbours of ratio
    1000 go on - its x must stay bit-equal to that of its own solve.  Sample 0 alone gives the bits of sample 0 in the batch of 3."""
    H, W = 45, 70
    rho, f, e, dx = problem(H, W)
    rho = rho.copy()
    rho[1] = 1.0
    p = (rho, f, e, dx)
    both, info = solve(*p, mask, preconditioner='scaled')
    again, info_again = solve(*p, mask, preconditioner='scaled')
    hard, info_hard = solve(*one(p, 0), mask, preconditioner='scaled')
    easy, info_easy = solve(*one(p, 1), mask, preconditioner='scaled')
    print(info, info_hard, info_easy)
    assert torch.equal(both, again) and all(np.array_equal(info[k], info_again[k]) for k in info)
    assert info['iterations'][0] > CHECK and info['iterations'][2] > CHECK and info_easy['iterations'][0] == CHECK
    assert torch.equal(both[0], hard[0]) and info['iterations'][0] == info_hard['iterations'][0]
    assert torch.equal(both[1], easy[0]) and info['iterations'][1] == CHECK
    assert info['relative_residual'][0] == info_hard['relative_residual'][0] and info['relative_residual'][1] == info_easy['relative_residual'][0]


def workspace_bytes(n, H, W, mask, scaled=True):
    from poisson_cnn_amd import _lib
    lib = _lib.load()
    if mask:
        fn = lib.pcnn_varcoef_bc_pcg_workspace_scaled if scaled else lib.pcnn_varcoef_bc_pcg_workspace
        return int(fn(c_int(n), c_int(H), c_int(W), c_int(mask)))
    fn = lib.pcnn_varcoef_pcg_workspace_scaled if scaled else lib.pcnn_varcoef_pcg_workspace
    return int(fn(c_int(n), c_int(H), c_int(W)))


def fill_free_blocks(H, W, mask, value):
    """Leaves `value` in the allocator's free blocks of the scaled solve's workspace size (tests/test_gpu_varcoef.py: fill_free_blocks)."""
    words = (workspace_bytes(N, H, W, mask) + 7) // 8
    held = [torch.full((words,), value, dtype=torch.float64, device='cuda') for _ in range(4)]
    torch.cuda.synchronize()
    del held
    probe = torch.empty((words,), dtype=torch.float64, device='cuda')
    seen = probe.clone()
    del probe
    return seen


@pytest.mark.parametrize('mask', MASKS)
def test_result_does_not_depend_on_what_the_workspace_held(mask):
    """The workspace - the new field s and the buffer s o r shares with z included - is not cleared: a solve into blocks that held NaN gives the bits
    of a solve into blocks that held zeros, from a zero start and from a start at the solution (every sample flagged at setup)."""
    H, W = 33, 47
    p = problem(H, W)
    guess = torch.tensor(np.stack([r[0] for r in twin(H, W, mask)])[:, None], dtype=torch.float64)
    runs = {}
    for value in (0.0, float('nan')):
        for name, kw in (('cold', {}), ('at the solution', {'initial_guesses': guess})):
            seen = fill_free_blocks(H, W, mask, value)
            assert bool(torch.isnan(seen).all()) == (value != 0.0)              # the allocator does hand the filled block back
            runs[name, value != 0.0] = solve(*p, mask, preconditioner='scaled', **kw)
    for name in ('cold', 'at the solution'):
        (clean, info), (dirty, info_dirty) = runs[name, False], runs[name, True]
        assert torch.isfinite(dirty).all() and np.isfinite(info_dirty['relative_residual']).all()
        assert torch.equal(clean, dirty) and info_dirty['converged'].all()
        assert all(np.array_equal(info[k], info_dirty[k]) for k in info)


# ----------------------------------------------------------------------------- 4. warm start
@pytest.mark.parametrize('mask', MASKS)
def test_a_start_at_the_solution_returns_after_no_iteration(mask):
    H, W = 33, 47
    p = problem(H, W)
    ref = twin(H, W, mask)
    guess = torch.tensor(np.stack([r[0] for r in ref])[:, None] + (3.0 if mask == 15 else 0.0), dtype=torch.float64)     # mask 15: any constant is in the null space
    warm, info = solve(*p, mask, preconditioner='scaled', check_start=True, initial_guesses=guess)
    print(info)
    assert (info['iterations'] == 0).all() and info['converged'].all()
    assert max(rel(warm[n, 0].cpu().numpy(), ref[n][0]) for n in range(N)) <= 2e-7
    # a start that is merely close - the solution rounded to fp32 - iterates, and arrives at the same solution
    rough = torch.tensor(np.stack([r[0] for r in ref])[:, None], dtype=torch.float32).to(torch.float64)
    near, info_near = solve(*p, mask, preconditioner='scaled', check_start=True, initial_guesses=rough)
    print(info_near)
    assert info_near['converged'].all() and (info_near['relative_residual'] <= 1e-10).all()
    assert max(rel(near[n, 0].cpu().numpy(), ref[n][0]) for n in range(N)) <= 2e-7


# ----------------------------------------------------------------------------- 5. refusals
def test_nan_and_nonpositive_density_are_refused_and_the_c_abi_checks_the_larger_workspace():
    from poisson_cnn_amd.dataset import _kernels as K
    from poisson_cnn_amd.ops import _p, handle
    H, W = 33, 47
    rho, f, e, dx = problem(H, W)
    for mask, at in ((0, (1, 5, 6)), (1, (1, 0, 6)), (15, (2, H - 1, W - 1))):            # interior; on the Neumann left edge; the Neumann corner
        for value in (np.nan, 0.0, -1.0):
            bad = rho.copy()
            bad[at] = value
            with pytest.raises(ValueError, match='positive'):
                solve(bad, f, e, dx, mask, preconditioner='scaled')
    with pytest.raises(ValueError, match='preconditioner'):
        solve(rho, f, e, dx, 0, preconditioner='jacobi')
    for mask in MASKS:
        i0, i1, j0, j1 = B.unknowns(H, W, mask)
        assert workspace_bytes(N, H, W, mask) - workspace_bytes(N, H, W, mask, scaled=False) == 8 * N * (i1 - i0 + 1) * (j1 - j0 + 1)
    assert workspace_bytes(N, 2, W, 0) == 0 and workspace_bytes(N, H, W, 16) == 0
    # a workspace of the plain size is too small for the scaled setup: refused before anything is launched
    ed = [dev(e[k]) for k in EDGES]
    scal, flags = torch.empty((N, 8), dtype=torch.float64, device='cuda'), torch.empty((N,), dtype=torch.int32, device='cuda')
    for mask in (0, 5):
        small = workspace_bytes(N, H, W, mask, scaled=False)
        ws = torch.empty((workspace_bytes(N, H, W, mask) + 7) // 8, dtype=torch.float64, device='cuda')
        with pytest.raises(RuntimeError, match='workspace'):
            if mask:
                bases = K._varcoef_bases(H, W, B.flags(mask), ws.device)
                handle().call('pcnn_varcoef_bc_pcg_setup_scaled', c_int(N), c_int(H), c_int(W), c_int(mask), _p(dev(rho)), _p(dev(f)), *[_p(t) for t in ed],
                              _p(dev(dx)), None, c_double(1e-10), *[_p(t) for t in bases], _p(ws), c_size_t(small), _p(scal), _p(flags))
            else:
                Sh, lh = K.dst_matrices(H, ws.device)
                Sw, lw = K.dst_matrices(W, ws.device)
                handle().call('pcnn_varcoef_pcg_setup_scaled', c_int(N), c_int(H), c_int(W), _p(dev(rho)), _p(dev(f)), *[_p(t) for t in ed], _p(dev(dx)), None,
                              c_double(1e-10), _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(small), _p(scal), _p(flags))


# ----------------------------------------------------------------------------- 6. the smooth density profile
@pytest.mark.parametrize('shape', [(3, 33, 47), (2, 97, 65), (1, 300, 300)])
def test_smooth_density_profile_matches_its_numpy_restatement(shape):
    """rho = lo + (hi - lo) (g - min g) / (max g - min g) per sample: 1e-6 relative to the fp64 restatement at every point (five fp32 roundings -
    difference, reciprocal, two products, a sum of two positive terms - are 5 x 2^-24 = 3e-7), min = lo and max = hi to one fp32 ulp, nothing
    outside [lo, hi].  33 x 47: one block per sample; 97 x 65: four; 300 x 300: 44, beyond one
    wave of partials.  A constant sample gives lo."""
    from poisson_cnn_amd.dataset import _kernels as K
    lo, hi = 1.0, 1000.0
    rng = np.random.default_rng(shape[1])
    g = np.stack([T.smooth_density(rng, shape[1], shape[2], -0.7, 1.3) * (n + 1) for n in range(shape[0])]).astype(np.float32)
    if shape[0] > 1:
        g[-1] = 0.25
    out = K.varcoef_density_smooth(dev(g), lo, hi)
    assert tuple(out.shape) == shape and out.dtype == torch.float32
    out = out.cpu().numpy()
    g64 = g.astype(np.float64)
    ulp = lambda v: float(np.spacing(np.float32(v)))
    for n in range(shape[0]):
        span = g64[n].max() - g64[n].min()
        if span == 0:
            assert np.array_equal(out[n], np.full(shape[1:], lo, dtype=np.float32))
            continue
        want = lo + (hi - lo) * (g64[n] - g64[n].min()) / span
        assert (np.abs(out[n] - want) <= 1e-6 * want).all()
        assert abs(float(out[n].min()) - lo) <= ulp(lo) and abs(float(out[n].max()) - hi) <= ulp(hi)
        assert out[n].min() >= lo and out[n].max() <= hi
    with pytest.raises(RuntimeError, match='lo <= hi'):
        K.varcoef_density_smooth(dev(g), 2.0, 1.0)


# ----------------------------------------------------------------------------- 7. generator and model, end to end
def test_generator_and_model_solve_run_end_to_end_with_the_scaled_preconditioner():
    from poisson_cnn_amd import dataset as D
    from tests import test_gpu_varcoef_model as VM
    H, W = 33, 47
    kw = dict(batch_size=2, batches_per_epoch=1, output_shape=(H, W), density_range=(1.0, 100.0), rhs_smoothness_range=(4, 7), density_smoothness_range=(3, 6), seed=9)
    gen = D.variable_density_dataset_generator(preconditioner='scaled', density_profile='smooth', **kw)
    (stack, dx), soln = gen[0]
    rhs, rho = stack[:, 0].cpu().numpy().astype(np.float64), stack[:, 1].cpu().numpy().astype(np.float64)
    d = dx[:, 0].cpu().numpy().astype(np.float64)
    zero = {k: np.zeros((2, W if k in ('left', 'right') else H)) for k in EDGES}
    ref = T.solve_batch(rho, rhs, zero, d)
    errs = [rel(soln[n, 0].cpu().numpy(), ref[n]) for n in range(2)]
    print('generator, smooth profile, scaled: rel-L2', errs, gen.last_info)
    assert max(errs) <= 2e-7 and gen.last_info['converged'].all()
    ulp = lambda v: float(np.spacing(np.float32(v)))
    assert np.abs(rho.min(axis=(1, 2)) - 1.0).max() <= ulp(1.0) and np.abs(rho.max(axis=(1, 2)) - 100.0).max() <= ulp(100.0)
    # the profile and the preconditioner change no draw: the same right-hand side and spacing as the default generator, whose rho is the kinked one
    (stack_abs, dx_abs), _ = D.variable_density_dataset_generator(**kw)[0]
    assert torch.equal(stack_abs[:, 0], stack[:, 0]) and torch.equal(dx_abs, dx) and not torch.equal(stack_abs[:, 1], stack[:, 1])
    plain = D.variable_density_dataset_generator(density_profile='smooth', **kw)
    (stack_p, _), soln_p = plain[0]
    assert torch.equal(stack_p, stack) and rel(soln_p.cpu().numpy(), soln.cpu().numpy()) <= 2e-7
    print('iterations: scaled', gen.last_info['iterations'], 'dst', plain.last_info['iterations'])
    # model.solve on that batch
    m = VM.build(VM.model_cfg(2, density_input=True))[0]
    warm, info = m.solve([stack, dx], return_info=True, compare_cold=True, preconditioner='scaled')
    cold, info_cold = m.solve([stack, dx], return_info=True, warm_start=False, preconditioner='scaled')
    print(info, info_cold)
    assert info['converged'].all() and info_cold['converged'].all() and np.array_equal(info['cold_iterations'], info_cold['iterations'])
    assert max(rel(warm[n, 0].cpu().numpy(), ref[n]) for n in range(2)) <= 2e-7 and max(rel(cold[n, 0].cpu().numpy(), ref[n]) for n in range(2)) <= 2e-7
    zeros = {k: dev(v) for k, v in zero.items()}
    assert torch.equal(cold, D.variable_density_poisson_solve(stack[:, 1].contiguous(), stack[:, 0].contiguous(), zeros, dx, preconditioner='scaled'))
    assert torch.equal(m.solve([stack, dx], preconditioner='dst'), m.solve([stack, dx]))
    with pytest.raises(ValueError, match='preconditioner'):
        m.solve([stack, dx], preconditioner='ilu')
