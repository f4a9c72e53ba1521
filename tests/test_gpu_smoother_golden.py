"""The Jacobi smoothers (one-sweep pair, fused any-stencil family with and without Neumann edges, variable-density family), both residual-loss
families and error_stats against tests/golden/smoother_parent.npz: what the commit BEFORE the two sweep families were put on one walker, one
tile frame, one launch chain and one block tree sum (csrc/sweep_common.h, pcnn_block_sum) returned for the same inputs.
tools/record_smoother_golden.py made the file and is the code that runs a case here too.

Bit for bit, every output: no arithmetic was reordered, so there is no tolerance.  Fields of more than R.FULL_MAX elements are held to the SHA-256
of their bytes (R.stored), smaller ones and those of the R.FULL cases to their values."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import record_smoother_golden as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def checked_inputs(H, W, N):
    """The recorder's inputs of a grid, once they are known to be those of the golden file."""
    g, d = golden(), R.inputs(H, W, N)
    for k, v in d.items():
        assert np.array_equal(R.stored(v), g['in/%dx%dx%d/%s' % (H, W, N, k)]), 'the recorder no longer draws the inputs of the golden file (%s)' % k
    return d


def test_the_cases_are_the_ones_the_golden_was_asked_for():
    from poisson_cnn_amd import ops
    assert all(ops.jacobi_k_max(*ss) == k for ss, k in R.FUSED_STENCILS.items()) and ops.varcoef_jacobi_k_max() == R.VARCOEF_K_MAX
    assert R.FUSED_STENCILS == {(3, 3): 8, (5, 3): 4, (9, 9): 2} and R.sweep_counts(8) == [1, 8, 9, 17] == R.VARCOEF_SWEEPS
    plain = {(c[1], c[2][:2]) for c in R.CASES if c[0] == 'fused' and c[4] == 0 and c[2][:2] != (13, 13)}
    assert plain == {((3, 3), g) for g in [(9, 9), (3, 70), (70, 3), (65, 130)]} | {(ss, g) for ss in [(5, 3), (9, 9)] for g in [(9, 9), (65, 130)]}
    for ss, k in R.FUSED_STENCILS.items():
        assert sorted(c[3] for c in R.CASES if c[0] == 'fused' and c[1] == ss and c[2] == (65, 130, 2) and c[4] == 0) == R.sweep_counts(k)
        for g in [(13, 13), (65, 130)]:
            assert all(('fused', ss, g + (2,), n, m) in R.CASES for m in (0, 5, 15) for n in (1, k, k + 1, 2 * k + 1))
    assert all(c[2][2] == 2 for c in R.CASES if c[0] in ('fused', 'sweep', 'varcoef'))
    assert [c[2] for c in R.CASES if c[0] == 'sweep'] == [(3, 3, 2), (65, 130, 2)]
    assert {(c[2], c[3]) for c in R.CASES if c[0] == 'varcoef'} == {((H, W, 2), n) for H, W in [(3, 3), (3, 70), (70, 3), (65, 130)] for n in (1, 8, 9, 17)}
    assert [c[2] for c in R.CASES if c[0] == 'varcoef_loss'] == [(3, 3, 3), (18, 66, 3), (19, 67, 3), (35, 131, 3)]
    assert [(c[1], c[2]) for c in R.CASES if c[0] == 'pi_loss'] == [((3, 3), (19, 67, 3)), ((5, 3), (19, 67, 3))]
    assert [c[2] for c in R.CASES if c[0] == 'error_stats'] == [(19, 67, 3)]
    outs = {k.rsplit('/', 1)[0] for k in golden() if k.startswith('out/')}
    assert outs == {'out/' + R.case_id(c) for c in R.CASES} and len(outs) == len(R.CASES)
    assert all(c in R.CASES and golden()['out/%s/fwd' % R.case_id(c)].shape == (2, 65, 130) for c in R.FULL) and len(R.FULL) == 2


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_bit_for_bit(case):
    g = golden()
    prefix = 'out/%s/' % R.case_id(case)
    want = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    got = R.run(case, checked_inputs(*case[2]))
    assert want and set(want) == set(got)
    for k, v in got.items():
        s = R.stored(v, case in R.FULL)
        assert s.dtype == want[k].dtype and s.shape == want[k].shape, k
        if s.dtype.kind == 'f':
            print('%s: %d of %d values differ from the golden' % (k, int((s != want[k]).sum()), s.size))
        assert np.array_equal(s, want[k]), k
