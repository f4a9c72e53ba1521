"""The variable-density solve with per-edge Dirichlet / Neumann boundaries (the *_bc_* entry points of poisson_cnn_amd/csrc/varcoef.hip, DESIGN.md
section 19) against the fp64 twin of tests/varcoef_bc_twin.py, whose own properties tests/test_varcoef_bc_reference.py checks without a GPU.

Bounds are those of tests/test_gpu_varcoef.py: 1e-12 relative for the operator (fp64 on both sides, a sum of five terms), 2e-7 rel-L2 for an fp32
solution of an fp64 solve, 1e-10 for the relative residual, iterations within one look (check_every) of the twin's recurrence."""
import functools
from ctypes import c_double, c_int, c_size_t

import numpy as np
import pytest
import torch

from tests import varcoef_bc_twin as B
from tests import varcoef_twin as T

pytestmark = pytest.mark.gpu
EDGES = B.EDGES
CHECK = 8
SOLVE_MASKS = [1, 2, 4, 8, 3, 12, 5, 10, 7, 15]


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def problem(seed, N, H, W, ratio):
    """float32-representable inputs of N samples; read, never written."""
    rng = np.random.default_rng(seed)
    rho = f32(np.stack([T.smooth_density(rng, H, W, 1.0, ratio) for _ in range(N)]))
    f = f32(rng.uniform(-1, 1, (N, H, W)))
    e = {k: f32(rng.uniform(-1, 1, (N, W if k in ('left', 'right') else H))) for k in EDGES}
    dx = f32(rng.uniform(5e-3, 5e-2, N))
    return rho, f, e, dx


def sample(e, n):
    return {k: v[n] for k, v in e.items()}


@functools.lru_cache(maxsize=None)
def twin(seed, N, H, W, ratio, mask):
    """Per sample: the direct solution, the twin recurrence's iteration count, the compatibility defect (mask 15)."""
    rho, f, e, dx = problem(seed, N, H, W, ratio)
    out = []
    for n in range(N):
        A, b = B.assemble(rho[n], dx[n], mask, sample(e, n), f[n])
        out.append((B.solve(rho[n], f[n], sample(e, n), dx[n], mask), B.pcg(A, b, H, W, mask, tol=1e-10)[1],
                    B.project(b, B.weights(H, W, mask))[1] if mask == 15 else 0.0))
    return out


def solve(rho, f, e, dx, mask, **kw):
    from poisson_cnn_amd import dataset as D
    return D.variable_density_poisson_solve(dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx), return_info=True, boundary_types=B.types(mask), **kw)


def kernel_solve(rho, f, e, dx, neumann, **kw):
    from poisson_cnn_amd.dataset import _kernels as K
    return K.varcoef_pcg_solve(dev(rho), dev(f), dev(e['left']), dev(e['right']), dev(e['bottom']), dev(e['top']), dev(dx), neumann=neumann, **kw)


# ----------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize('H,W', [(3, 4), (18, 66), (19, 70)])
def test_operator_matches_the_twin_matrix_for_every_mask(H, W):
    """3x4: one or two unknowns per axis, every node next to an edge; 18x66: exactly one 16 x 64 tile at mask 0, four tiles with 2-wide tails at
    mask 15; 19x70: partial tiles at every mask."""
    from poisson_cnn_amd.dataset import _kernels as K
    N = 2
    rho, _, _, dx = problem(H * W, N, H, W, 100.0)
    rng = np.random.default_rng(H + W)
    worst = [0.0, 0.0, 0.0]
    for mask in range(16):
        i0, i1, j0, j1 = B.unknowns(H, W, mask)
        mh, mw = i1 - i0 + 1, j1 - j0 + 1
        w = B.weights(H, W, mask)
        u, v = rng.standard_normal((2, N, mh, mw))
        ref = np.stack([(B.assemble(rho[n], dx[n], mask)[0] @ u[n].ravel()).reshape(mh, mw) for n in range(N)])
        q, pq = K.varcoef_apply(dev(rho), dev(dx), dev(u, torch.float64), neumann=B.flags(mask))
        assert tuple(q.shape) == (N, mh, mw)
        q = q.cpu().numpy()
        ref_pq = np.einsum('ij,nij,nij->n', w, u, ref)
        err, err_pq = rel(q, ref), np.abs(pq.cpu().numpy() - ref_pq).max() / np.abs(ref_pq).max()
        qv = K.varcoef_apply(dev(rho), dev(dx), dev(v, torch.float64), neumann=B.flags(mask))[0].cpu().numpy()
        uAv, vAu = np.einsum('ij,nij,nij->n', w, u, qv), np.einsum('ij,nij,nij->n', w, v, q)
        sym = (np.abs(uAv - vAu) / np.abs(uAv)).max()
        worst = [max(a, c) for a, c in zip(worst, (err, err_pq, sym))]
        assert err <= 1e-12 and err_pq <= 1e-12 and sym <= 1e-12, (mask, err, err_pq, sym)
    print('%dx%d: operator rel-L2 %.2e, weighted p.q rel %.2e, symmetry defect %.2e (worst over the 16 masks)' % (H, W, *worst))


# ----------------------------------------------------------------------------- 2. solve
@pytest.mark.parametrize('H,W', [(19, 70), (33, 40)])
@pytest.mark.parametrize('mask', SOLVE_MASKS)
def test_solve_matches_the_direct_sparse_solve(mask, H, W):
    key = (H + W, 2, H, W, 10.0)
    rho, f, e, dx = problem(*key)
    ref = twin(*key, mask)
    soln, info = solve(rho, f, e, dx, mask, tol=1e-10)
    assert tuple(soln.shape) == (2, 1, H, W) and soln.dtype == torch.float32
    s = soln[:, 0].cpu().numpy().astype(np.float64)
    errs = [rel(s[n], ref[n][0]) for n in range(2)]
    print('mask %d %dx%d: rel-L2 %s, twin iterations %s, %s' % (mask, H, W, errs, [r[1] for r in ref], info))
    assert max(errs) <= 2e-7
    assert info['converged'].all() and (info['relative_residual'] <= 1e-10).all()
    for n in range(2):
        assert info['iterations'][n] % CHECK == 0
        assert info['iterations'][n] <= -(-ref[n][1] // CHECK) * CHECK + CHECK, (n, ref[n][1], info['iterations'][n])
    if mask != 15:
        assert (info['compatibility_defect'] == 0).all() and (info['rhs_shift'] == 0).all()
    # a Dirichlet edge holds its values, rows 0 / H-1 first
    nl, nr, nb, nt = B.flags(mask)
    if not nl:
        assert np.array_equal(s[:, 0, :], e['left'])
    if not nr:
        assert np.array_equal(s[:, -1, :], e['right'])
    if not nb:
        assert np.array_equal(s[:, 1:-1, 0], e['bottom'][:, 1:-1])
    if not nt:
        assert np.array_equal(s[:, 1:-1, -1], e['top'][:, 1:-1])


# ----------------------------------------------------------------------------- 3. constant density
@pytest.mark.parametrize('mask', SOLVE_MASKS)
def test_constant_density_is_the_mixed_solve_in_one_look(mask):
    from poisson_cnn_amd import dataset as D
    _, f, e, dx = problem(3, 2, 19, 70, 10.0)
    soln, info = solve(np.full_like(f, 2.5), f, e, dx, mask)
    ref = D.mixed_bc_poisson_solve(dev(2.5 * f), {k: dev(v) for k, v in e.items()}, dev(dx), B.types(mask))
    err = rel(soln.cpu().numpy(), ref.cpu().numpy())
    print('mask %d, rho = 2.5 against mixed_bc_poisson_solve: rel-L2 %.3e' % (mask, err), info)
    assert err <= 2e-7
    assert (info['iterations'] == CHECK).all() and info['converged'].all()        # the preconditioner is exact: converged at the first look


# ----------------------------------------------------------------------------- 4. mask 0 through the new entry points
def test_mask_0_through_the_bc_entry_points_gives_the_bits_of_the_dirichlet_ones():
    from poisson_cnn_amd import dataset as D
    rho, f, e, dx = problem(4, 3, 45, 70, 100.0)
    d = lambda: (dev(rho), dev(f), {k: dev(v) for k, v in e.items()}, dev(dx))
    today, info_today = D.variable_density_poisson_solve(*d(), return_info=True)
    typed, info_typed = D.variable_density_poisson_solve(*d(), return_info=True, boundary_types={k: 'dirichlet' for k in EDGES})
    assert torch.equal(today, typed) and set(info_today) == set(info_typed)
    old, info_old = kernel_solve(rho, f, e, dx, None)
    new, info_new = kernel_solve(rho, f, e, dx, (False,) * 4)                     # the *_bc_* kernels at mask 0
    assert torch.equal(old, today[:, 0]) and torch.equal(old, new)
    assert info_old['iterations'].max() > CHECK                                   # a real solve, not one look
    assert set(info_old) == set(info_new)
    for k in info_old:
        assert np.array_equal(info_old[k], info_new[k]), k
    for k in info_today:
        assert np.array_equal(info_today[k], info_typed[k]) and np.array_equal(info_today[k], info_new[k]), k


# ----------------------------------------------------------------------------- 5. all four edges Neumann
def test_all_neumann_projects_incompatible_data_and_returns_the_zero_mean_solution():
    H, W = 19, 70
    rho, f, e, dx = problem(H + W, 2, H, W, 10.0)
    f = f32(f + 0.5)                                                              # deliberately incompatible: a right-hand side with a large mean
    ref = []
    for n in range(2):
        A, b = B.assemble(rho[n], dx[n], 15, sample(e, n), f[n])
        ref.append((B.solve(rho[n], f[n], sample(e, n), dx[n], 15), 0, B.project(b, B.weights(H, W, 15))[1]))
    soln, info = solve(rho, f, e, dx, 15, check_start=True)
    s = soln[:, 0].cpu().numpy().astype(np.float64)
    w = B.weights(H, W, 15)
    print('defect', info['compatibility_defect'], [r[2] for r in ref], 'shift', info['rhs_shift'])
    for n in range(2):
        assert 0.01 < ref[n][2] <= 1.0
        assert abs(info['compatibility_defect'][n] - ref[n][2]) <= 1e-10
        assert abs((w * s[n]).sum()) / (w.sum() * np.abs(s[n]).max()) <= 1e-6
        assert rel(s[n], ref[n][0]) <= 2e-7
        # the solution satisfies the discrete equation of f + rhs_shift
        A, b = B.assemble(rho[n], dx[n], 15, sample(e, n), f[n] + info['rhs_shift'][n])
        assert abs((w.ravel() * b).sum()) <= 1e-9 * np.abs(w.ravel() * b).sum()
    assert info['iterations'].min() >= CHECK
    warm, info_warm = solve(rho, f, e, dx, 15, check_start=True, initial_guesses=torch.tensor(np.stack([r[0] for r in ref])[:, None] + 3.0, dtype=torch.float64))
    print(info_warm)
    assert (info_warm['iterations'] == 0).all() and info_warm['converged'].all()  # the constant is in the null space: the start meets the tolerance
    assert max(rel(warm[n, 0].cpu().numpy(), ref[n][0]) for n in range(2)) <= 2e-7            # and the mean is removed at the finish


# ----------------------------------------------------------------------------- 6. order of accuracy
def manufactured(n, mask):
    """u = exp(0.7 x) sin(1.3 y + 0.4) + x y^2, rho = 1 + 2 x + 1.5 y^2 + sin(2 x y) on the unit square (x along axis 0); f = div((1/rho) grad u)
    and g = du/dn from the analytic derivatives -> max |error| of the device solve."""
    x, y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing='ij')
    ex, sn, cs = np.exp(0.7 * x), np.sin(1.3 * y + 0.4), np.cos(1.3 * y + 0.4)
    u = ex * sn + x * y ** 2
    ux, uy = 0.7 * ex * sn + y ** 2, 1.3 * ex * cs + 2 * x * y
    lap = (0.49 - 1.69) * ex * sn + 2 * x
    rho = 1 + 2 * x + 1.5 * y ** 2 + np.sin(2 * x * y)
    rx, ry = 2 + 2 * y * np.cos(2 * x * y), 3 * y + 2 * x * np.cos(2 * x * y)
    f = lap / rho - (rx * ux + ry * uy) / rho ** 2
    nl, nr, nb, nt = B.flags(mask)
    e = {'left': -ux[0] if nl else u[0], 'right': ux[-1] if nr else u[-1], 'bottom': -uy[:, 0] if nb else u[:, 0], 'top': uy[:, -1] if nt else u[:, -1]}
    soln, info = solve(rho[None], f[None], {k: v[None] for k, v in e.items()}, np.array([1.0 / (n - 1)]), mask)
    assert info['converged'].all()
    return np.abs(soln[0, 0].cpu().numpy().astype(np.float64) - u).max()


@pytest.mark.parametrize('mask', [1, 10, 7])
def test_manufactured_solution_converges_at_second_order(mask):
    """The half-cell Neumann term 2 g / (rho_c h) is second order (ratio 3.98-4.01 in fp64); the mirrored ghost node's 2 beta_in g / h stops at 2.00."""
    e33, e65 = manufactured(33, mask), manufactured(65, mask)
    print('mask %d: max error 33^2 %.4e, 65^2 %.4e, ratio %.4f' % (mask, e33, e65, e33 / e65))
    assert 3.5 <= e33 / e65 <= 4.5


# ----------------------------------------------------------------------------- 7. independence and determinism
def test_a_sample_does_not_depend_on_its_batch_and_two_runs_are_bit_equal():
    H, W = 45, 70
    rho, f, e, dx = problem(4, 2, H, W, 100.0)
    rho = rho.copy()
    rho[1] = 1.0
    one = lambda n: (rho[n:n + 1], f[n:n + 1], {k: v[n:n + 1] for k, v in e.items()}, dx[n:n + 1])
    both, info = solve(rho, f, e, dx, 5)
    again, info_again = solve(rho, f, e, dx, 5)
    hard, info_hard = solve(*one(0), 5)
    easy, info_easy = solve(*one(1), 5)
    print(info, info_hard, info_easy)
    assert torch.equal(both, again) and all(np.array_equal(info[k], info_again[k]) for k in info)
    assert info['iterations'][0] > CHECK and info_easy['iterations'][0] == CHECK      # the easy sample sat frozen while the hard one went on
    assert torch.equal(both[0], hard[0]) and info['iterations'][0] == info_hard['iterations'][0]
    assert torch.equal(both[1], easy[0]) and info['iterations'][1] == CHECK


def fill_free_blocks(N, H, W, mask, value):
    """Leaves `value` in the allocator's free blocks of the solve's workspace size (tests/test_gpu_varcoef.py: fill_free_blocks)."""
    from poisson_cnn_amd import _lib
    words = (int(_lib.load().pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(mask))) + 7) // 8
    held = [torch.full((words,), value, dtype=torch.float64, device='cuda') for _ in range(4)]
    torch.cuda.synchronize()
    del held
    probe = torch.empty((words,), dtype=torch.float64, device='cuda')
    seen = probe.clone()
    del probe
    return seen


@pytest.mark.parametrize('mask', [5, 15])
def test_result_does_not_depend_on_what_the_workspace_held(mask):
    """The workspace is not cleared: a solve into blocks that held NaN gives the bits of a solve into blocks that held zeros - from a zero start and
    from a start at the solution (flagged at setup).  mask 15 adds the projection pass and the mean removal, which use the workspace too."""
    key = (33 + 40, 2, 33, 40, 10.0)
    rho, f, e, dx = problem(*key)
    guess = torch.tensor(np.stack([r[0] for r in twin(*key, mask)])[:, None], dtype=torch.float64)
    runs = {}
    for value in (0.0, float('nan')):
        for name, kw in (('cold', {}), ('at the solution', {'initial_guesses': guess})):
            seen = fill_free_blocks(2, 33, 40, mask, value)
            assert bool(torch.isnan(seen).all()) == (value != 0.0)              # the allocator does hand the filled block back
            runs[name, value != 0.0] = solve(rho, f, e, dx, mask, **kw)
    for name in ('cold', 'at the solution'):
        (clean, info), (dirty, info_dirty) = runs[name, False], runs[name, True]
        assert torch.isfinite(dirty).all() and np.isfinite(info_dirty['relative_residual']).all()
        assert torch.equal(clean, dirty) and info_dirty['converged'].all()
        assert all(np.array_equal(info[k], info_dirty[k]) for k in info)


# ----------------------------------------------------------------------------- 8. refusals through the C ABI
def test_c_abi_refusals():
    from poisson_cnn_amd import _lib
    from poisson_cnn_amd.dataset import _kernels as K
    from poisson_cnn_amd.ops import _p, handle
    lib = _lib.load()
    N, H, W = 2, 9, 12
    rho, f, e, dx = problem(8, N, H, W, 10.0)
    assert lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(16)) == 0
    assert lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(2), c_int(W), c_int(5)) == 0
    assert lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(15)) > lib.pcnn_varcoef_pcg_workspace(c_int(N), c_int(H), c_int(W))

    def setup(mask, Hc=H, rho_=rho, shrink=0):
        r, g = dev(rho_[:, :Hc].copy()), dev(f[:, :Hc].copy())
        ed = [dev(e['left']), dev(e['right']), dev(e['bottom'][:, :Hc].copy()), dev(e['top'][:, :Hc].copy())]
        nbytes = int(lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(15)))          # the largest of any mask at the full shape
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
        scal, flags = torch.empty((N, 8), dtype=torch.float64, device='cuda'), torch.empty((N,), dtype=torch.int32, device='cuda')
        bases = K._varcoef_bases(max(Hc, 3), W, B.flags(mask & 15), r.device)
        need = int(lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(Hc), c_int(W), c_int(mask)))
        handle().call('pcnn_varcoef_bc_pcg_setup', c_int(N), c_int(Hc), c_int(W), c_int(mask), _p(r), _p(g), *[_p(t) for t in ed], _p(dev(dx)), None, c_double(1e-10),
                      *[_p(t) for t in bases], _p(ws), c_size_t(need - shrink if need else nbytes), _p(scal), _p(flags))
        return scal

    with pytest.raises(RuntimeError, match='neumann_mask'):
        setup(16)
    with pytest.raises(RuntimeError, match='unsupported'):
        setup(5, Hc=2)
    with pytest.raises(RuntimeError, match='workspace'):
        setup(5, shrink=8)
    with pytest.raises(RuntimeError, match='neumann_mask'):
        handle().call('pcnn_varcoef_bc_apply', c_int(N), c_int(H), c_int(W), c_int(-1), _p(dev(rho)), _p(dev(dx)), _p(dev(np.zeros((N, H, W)), torch.float64)),
                      _p(dev(np.zeros((N, H, W)), torch.float64)), _p(dev(np.zeros(N), torch.float64)))
    assert (setup(5)[:, K.VARCOEF_SCALARS['rho_min']] > 0).all()                  # the same call with nothing wrong goes through
    bad = rho.copy()
    bad[1, 0, 6] = 0.0                                                            # a node of the (Neumann) left edge: it is read now
    assert float(setup(5, rho_=bad)[1, K.VARCOEF_SCALARS['rho_min']]) == 0.0      # the C ABI reports the minimum ...
    with pytest.raises(ValueError, match='positive'):
        solve(bad, f, e, dx, 5)                                                   # ... and the caller refuses it
    bad[1, 0, 6] = np.nan
    with pytest.raises(ValueError, match='positive'):
        solve(bad, f, e, dx, 1)


# ----------------------------------------------------------------------------- 9. generator
def test_generator_batches():
    from poisson_cnn_amd import dataset as D
    kw = dict(batch_size=2, batches_per_epoch=1, output_shape=(33, 40), density_range=(1.0, 10.0), rhs_smoothness_range=(4, 7), density_smoothness_range=(3, 6),
              boundaries='random', seed=9)
    unpack = lambda inp: (inp[0][:, 0].cpu().numpy().astype(np.float64), inp[0][:, 1].cpu().numpy().astype(np.float64),
                          {k: v[:, 0].cpu().numpy().astype(np.float64) for k, v in zip(('left', 'top', 'right', 'bottom'), inp[1:5])},
                          inp[5][:, 0].cpu().numpy().astype(np.float64))
    # two Neumann edges: the batch satisfies the twin's system
    gen = D.variable_density_dataset_generator(boundary_types={'left': 'neumann', 'top': 'neumann'}, **kw)
    inp, soln = gen[0]
    rhs, rho, e, dx = unpack(inp)
    ref = B.solve_batch(rho, rhs, e, dx, 9)
    errs = [rel(soln[n, 0].cpu().numpy(), ref[n]) for n in range(2)]
    print('generator, left and top Neumann: rel-L2', errs)
    assert max(errs) <= 2e-7 and gen.last_info['converged'].all()
    # the draws do not depend on the types: the same inputs as the all-Dirichlet generator, whose batch is the one of a generator without the argument
    plain, typed = D.variable_density_dataset_generator(**kw), D.variable_density_dataset_generator(boundary_types=None, **kw)
    (inp_p, soln_p), (inp_t, soln_t) = plain[0], typed[0]
    assert torch.equal(soln_p, soln_t) and all(torch.equal(a, c) for a, c in zip(inp_p, inp_t))
    assert all(torch.equal(a, c) for a, c in zip(inp_p, inp))
    ref0 = T.solve_batch(rho, rhs, e, dx)
    assert max(rel(soln_p[n, 0].cpu().numpy(), ref0[n]) for n in range(2)) <= 2e-7
    # all four Neumann: the right-hand side handed out is the projected one, the drawn one plus the solver's shift, and (input, soln) satisfy the equation
    gen15 = D.variable_density_dataset_generator(boundary_types={k: 'neumann' for k in EDGES}, **kw)
    inp15, soln15 = gen15[0]
    rhs15, rho15, e15, dx15 = unpack(inp15)
    shift = gen15.last_info['rhs_shift']
    assert np.abs(shift).min() > 0 and np.array_equal(rho15, rho)
    assert np.array_equal(rhs15.astype(np.float32), (dev(rhs) + dev(shift).view(2, 1, 1)).cpu().numpy())
    w = B.weights(33, 40, 15)
    for n in range(2):
        A, b = B.assemble(rho15[n], dx15[n], 15, sample(e15, n), rhs15[n])
        assert B.project(b, w)[1] <= 1e-6                                         # compatible up to the fp32 rounding of the shifted rhs
        assert rel(soln15[n, 0].cpu().numpy(), B.solve(rho15[n], rhs15[n], sample(e15, n), dx15[n], 15)) <= 2e-7
    # boundaries = 'zero': a Neumann edge gets g = 0
    soln0, frho0 = D.variable_density_dataset_generator(batch_size=1, output_shape=(20, 24), boundaries='zero', return_keras_style=False, seed=1,
                                                        boundary_types={'right': 'neumann'})[0]
    assert float(soln0[:, :, 0].abs().max()) == 0.0 and float(soln0[:, :, -1, 1:-1].abs().max()) > 0.0
