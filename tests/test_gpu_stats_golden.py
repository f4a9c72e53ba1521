"""ops.error_stats and ops.varcoef_error_stats against tests/golden/stats_parent.npz: the (N, 8) rows that the commit BEFORE the two statistics
kernels became one template over the residual (csrc/error_stats.hip, csrc/flux_form.h) returned for the same inputs.
tools/record_stats_golden.py made the file and is the code that runs a case here too.

Bit for bit, every row: no arithmetic was reordered, so there is no tolerance."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import record_stats_golden as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def checked_inputs(H, W):
    """The recorder's inputs of a grid, once they are known to be those of the golden file."""
    g, d = golden(), R.inputs(H, W)
    for k, v in d.items():
        assert np.array_equal(R.stored(v), g['in/%dx%d/%s' % (H, W, k)]), 'the recorder no longer draws the inputs of the golden file (%s)' % k
    return d


def test_the_cases_are_the_ones_the_golden_was_asked_for():
    assert R.N == 3 and R.OPS == ('error_stats', 'varcoef_error_stats')
    with_rhs = {(c[0], c[1]) for c in R.CASES if c[1][0] >= 3}
    assert with_rhs == {(op, g) for op in R.OPS for g in [(3, 3), (5, 67), (70, 5), (130, 33), (65, 130)]}
    for op, g in with_rhs:                                                       # target and rhs, target only, rhs only, neither
        assert sorted((c[2], c[3]) for c in R.CASES if c[:2] == (op, g)) == [(False, False), (False, True), (True, False), (True, True)]
    small = [c for c in R.CASES if c[1][0] < 3]
    assert {(c[0], c[1]) for c in small} == {(op, g) for op in R.OPS for g in [(2, 5), (1, 1)]} and not any(c[3] for c in small)
    assert len(set(R.CASES)) == len(R.CASES) == 48
    outs = {k for k in golden() if k.startswith('out/')}
    assert outs == {'out/' + R.case_id(c) for c in R.CASES} and len(outs) == len(R.CASES)
    for H, W in {c[1] for c in R.CASES}:
        d = checked_inputs(H, W)
        assert len({float(v) for v in d['dx2'].ravel()}) == 2 * R.N and d['rho'].min() >= 1.0 and d['rho'].max() <= 10.0


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_bit_for_bit(case):
    want = golden()['out/' + R.case_id(case)]
    got = R.run(case, checked_inputs(*case[1]))
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (R.N, 8)
    print('%d of %d values differ from the golden' % (int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    target, rhs = case[2], case[3]
    assert np.all(got[:, :5] != 0) if target else np.all(got[:, :5] == 0)        # the golden is not a file of zeros
    assert np.all(got[:, 5:] != 0) if rhs else np.all(got[:, 5:] == 0)
