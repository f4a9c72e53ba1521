"""The four finite-difference Poisson solvers and the two seeded FD generators against tests/golden/fd_solver_parent.npz: what the commit
BEFORE the solvers were folded into one build kernel, one eigenvalue division, one ring / interior writer and one transform helper returned
for the same inputs (tools/record_fd_solver_golden.py made the file and is the code that runs a case here too).

Bit for bit: both Dirichlet routes, the variable-density solve with its iteration counts and residuals, every generator tensor that does not
come out of the mixed solve.  The mixed solve adds the same four edge terms in another order (bottom, top, left, right - the Dirichlet kernel's)
at unknowns that touch a row edge and a column edge: three fp64 additions reordered move the right-hand side by a few 2^-52, the solve amplifies
that by at most the condition number ~ n^2, about 1e-13 at these sizes, so the stored fp32 value moves only where the fp64 value sits on a
rounding boundary - by at most one unit in the last place, which is the bound below."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import record_fd_solver_golden as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case(grid, kind):
    """(inputs from the golden file, recorded outputs, outputs of this build) of one solve."""
    H, W, N = grid
    g = golden()
    d = {k: g['in/%dx%dx%d/%s' % (H, W, N, k)] for k in ('rhs', 'dx', 'rho', 'guess') + R.EDGES}
    for k, v in R.inputs(H, W, N).items():
        assert np.array_equal(v, d[k]), 'the recorder no longer draws the inputs of the golden file (%s)' % k
    prefix = 'out/%dx%dx%d/%s/' % (H, W, N, R.tag(kind))
    want = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    got = R.solve(kind, d)
    assert want and set(want) == set(got)
    return d, want, got


def within_one_ulp(new, old):
    assert new.dtype == np.float32 and old.dtype == np.float32 and new.shape == old.shape
    diff, ulp = np.abs(new.astype(np.float64) - old.astype(np.float64)), np.spacing(np.maximum(np.abs(new), np.abs(old))).astype(np.float64)
    print('max |new - golden| / ulp = %.3g, points that differ: %d of %d' % (float((diff / ulp).max()), int((diff > 0).sum()), diff.size))
    return bool((diff <= ulp).all())


def ring_holds(soln, d, neumann=(False, False, False, False)):
    """Dirichlet rows 0 / H-1 equal left / right corners included; Dirichlet columns equal bottom / top away from the corners those rows own."""
    nl, nr, nb, nt = neumann
    ok = (nl or np.array_equal(soln[:, 0, :], d['left'])) and (nr or np.array_equal(soln[:, -1, :], d['right']))
    rows = slice(0 if nl else 1, soln.shape[1] if nr else -1)
    return ok and (nb or np.array_equal(soln[:, rows, 0], d['bottom'][:, rows])) and (nt or np.array_equal(soln[:, rows, -1], d['top'][:, rows]))


def _id(v):
    return R.tag(v) if isinstance(v, str) or v[0] == 'mixed' else 'x'.join(map(str, v))


DIRICHLET = [(grid, kind) for grid, kinds in R.GRIDS.items() for kind in kinds if kind in ('gemm', 'fft')]
VARCOEF = [(grid, kind) for grid, kinds in R.GRIDS.items() for kind in kinds if kind in ('varcoef', 'varcoef_guess')]
MIXED = [(grid, kind) for grid, kinds in R.GRIDS.items() for kind in kinds if not isinstance(kind, str)]


def test_the_cases_are_the_ones_the_golden_was_asked_for():
    assert [c for c in DIRICHLET if c[1] == 'gemm'] == [(g, 'gemm') for g in ((3, 3, 2), (3, 8, 2), (8, 3, 2), (9, 7, 3), (33, 47, 2))]
    assert [c for c in DIRICHLET if c[1] == 'fft'] == [((9, 7, 3), 'fft'), ((33, 47, 2), 'fft')]
    assert len(VARCOEF) == 4 and {g for g, _ in VARCOEF} == {(9, 7, 3), (33, 47, 2)}
    assert sorted(k[1] for g, k in MIXED if g == (6, 5, 2)) == sorted(R.ALL_MASKS) and len(R.ALL_MASKS) == 16
    assert [k[1] for g, k in MIXED if g == (33, 47, 2)] == [(False, True, True, False), (True, True, True, True)]


@pytest.mark.parametrize('grid,kind', DIRICHLET, ids=_id)
def test_dirichlet_routes_bit_for_bit(grid, kind):
    d, want, got = case(grid, kind)
    assert np.array_equal(got['soln'], want['soln'])
    assert ring_holds(got['soln'], d)


@pytest.mark.parametrize('grid,kind', VARCOEF, ids=_id)
def test_variable_density_bit_for_bit(grid, kind):
    d, want, got = case(grid, kind)
    for k in ('soln', 'iterations', 'converged', 'relative_residual'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert bool(got['converged'].all())
    assert ring_holds(got['soln'], d)


@pytest.mark.parametrize('grid,kind', MIXED, ids=_id)
def test_mixed_route_within_one_ulp(grid, kind):
    d, want, got = case(grid, kind)
    assert within_one_ulp(got['soln'], want['soln'])
    assert ring_holds(got['soln'], d, kind[1])


def test_seeded_generators():
    g = golden()
    new = R.generator_batches()
    assert set(new) == {k for k in g if k.startswith('gen/')}
    for k, v in new.items():
        if k.startswith('gen/numerical_neumann_left/') and k.endswith('/5'):         # the solution of the mixed solve; rhs and edges stay exact
            assert within_one_ulp(v, g[k]), k
        else:
            assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k
