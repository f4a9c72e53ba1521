"""Homogeneous_Poisson_NN_Legacy's forward and backward on the tiny model, and the boundary-ring operators, against
tests/golden/hpnn_merge_parent.npz: what the commit BEFORE the eight-branch merge moved into models._BottleneckMerge (one branch API, one plan) and
before the two ring kernel pairs became one returned for the same inputs.  tools/record_hpnn_merge_golden.py made the file and is the code that
runs a case here too.

Bit for bit: no launch, no kernel's arithmetic and no order on a stream changed, so there is no tolerance.  The prediction is held to its values;
the flat gradient to its values or, where the file would have outgrown the largest committed golden, to its SHA-256 - and then one float64 sum per
parameter names the layers that differ."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import record_hpnn_merge_golden as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_cases_are_the_ones_the_golden_was_asked_for():
    assert R.N == 2 and {k: v[:2] + v[3:] for k, v in R.CASES.items()} == {
        'dirichlet_36x40': (36, 40, True), 'neumann_48x48': (48, 48, True), 'one_neumann_edge_enforce_36x40': (36, 40, True),
        'dirichlet_36x40_one_stream': (36, 40, False)}
    assert R.CASES['dirichlet_36x40'][2] == R.CASES['dirichlet_36x40_one_stream'][2] == {'bc_type': 'dirichlet'}
    assert R.CASES['neumann_48x48'][2] == {'bc_type': 'neumann'}
    assert R.CASES['one_neumann_edge_enforce_36x40'][2] == {'bc_type': {'left': 'neumann'}, 'smoother_boundaries': 'enforce', 'postsmoother_iterations': 2}
    assert R.RING_SHAPES == [(3, 3), (3, 5), (4, 4), (5, 7)]
    g = golden()
    assert {k.split('/')[1] for k in g if k.startswith('model/')} == set(R.CASES)
    assert {k.rsplit('/', 1)[0] for k in g if k.startswith('ring/')} == {'ring/%dx%d/flag%d' % (H, W, f) for H, W in R.RING_SHAPES for f in (0, 1)}


@pytest.mark.parametrize('name', list(R.CASES))
def test_model_bit_for_bit(name):
    g = golden()
    pred, grads = R.run_model(name)
    want = g['model/%s/pred' % name]
    assert pred.dtype == want.dtype == np.float32 and pred.shape == want.shape and float(np.abs(want).max()) > 0
    print('prediction: %d of %d values differ from the golden' % (int((pred != want).sum()), pred.size))
    assert np.array_equal(pred, want)
    full = 'model/%s/grad' % name in g
    got = R.gradient_record(grads, full)
    if full:
        assert got['grad'].dtype == np.float32 and np.array_equal(got['grad'], g['model/%s/grad' % name])
        return
    assert list(got['grad_names']) == list(g['model/%s/grad_names' % name])
    sums = g['model/%s/grad_sums' % name]
    assert np.abs(sums).max() > 0
    differ = [str(n) for n, a, b in zip(got['grad_names'], got['grad_sums'], sums) if a != b]
    print('parameters whose gradient sum differs from the golden:', differ)
    assert not differ
    assert np.array_equal(got['grad_sha256'], g['model/%s/grad_sha256' % name])


def test_one_stream_case_is_the_streamed_case():
    """The golden itself: the parent's gradient and prediction did not depend on the branch streams."""
    g = golden()
    for k in ('pred', 'grad_sha256', 'grad'):
        a, b = 'model/dirichlet_36x40/' + k, 'model/dirichlet_36x40_one_stream/' + k
        assert (a in g) == (b in g) and (a not in g or np.array_equal(g[a], g[b]))


@pytest.mark.parametrize('H,W', R.RING_SHAPES)
def test_ring_mask_path_is_the_flag_pair_of_the_parent(H, W):
    from poisson_cnn_amd import ops
    g = golden()
    for flag, mask in ((0, 0), (1, 15)):
        for path, arg in (('mask', mask), ('flag', bool(flag))):
            got = R.run_ring(H, W, ops.bc_ring_edges_fwd, ops.bc_ring_edges_bwd, arg) if path == 'mask' else R.run_ring(H, W, ops.bc_ring_fwd, ops.bc_ring_bwd, arg)
            for k, v in got.items():
                want = g['ring/%dx%d/flag%d/%s' % (H, W, flag, k)]
                assert v.dtype == want.dtype == np.float32 and v.shape == want.shape == (R.N, H, W, 1)
                assert v.tobytes() == want.tobytes(), (path, flag, k)          # bytes: the sign of a zero counts
        assert float(np.abs(g['ring/%dx%d/flag%d/bwd' % (H, W, flag)]).max()) > 0
