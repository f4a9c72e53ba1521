"""Records what ops.error_stats and ops.varcoef_error_stats return, for tests/test_gpu_stats_golden.py: inputs drawn from a seeded numpy generator
(rounded to fp32) and the (N, 8) rows of the GPU run, in tests/golden/stats_parent.npz.  Only poisson_cnn_amd.ops is used, so the same file runs on
any commit: the committed golden is the run of the commit BEFORE the two statistics kernels became one template over the residual
(csrc/error_stats.hip, csrc/flux_form.h), and the test holds the present code to it bit for bit.

    python tools/record_stats_golden.py [out.npz]

The test imports `CASES`, `inputs` and `run` from here, so golden and test cannot drift apart in how a case is run.  The inputs are regenerated
from the seed; the file holds them as values up to FULL_MAX elements and as the SHA-256 of dtype, shape and bytes above, so a generator that drifts
is caught."""
import functools
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'stats_parent.npz')
FULL_MAX = 1024
N = 3
# 3 x 3: one interior node; 5 x 67: the lane stride (64) is taken twice, and the column tail; 70 x 5: two rows per band, trailing empty bands;
# 130 x 33: three rows per band, neighbour rows belong to other workgroups; 65 x 130: two rows per band with 31 empty bands
RHS_GRIDS = [(3, 3), (5, 67), (70, 5), (130, 33), (65, 130)]
NO_RHS_GRIDS = [(2, 5), (1, 1)]                # no interior: allowed without rhs only
OPS = ('error_stats', 'varcoef_error_stats')
FIELDS = [(True, True), (True, False), (False, True), (False, False)]          # (target given, rhs given)

CASES = [(op, (H, W), t, f) for op in OPS for H, W in RHS_GRIDS for t, f in FIELDS]
CASES += [(op, (H, W), t, False) for op in OPS for H, W in NO_RHS_GRIDS for t in (True, False)]


def case_id(case):
    op, (H, W), t, f = case
    return '%s/%dx%d/%s' % (op, H, W, {(True, True): 'both', (True, False): 'target', (False, True): 'rhs', (False, False): 'neither'}[(t, f)])


def stored(a):
    """The form an array takes in the golden file."""
    a = np.ascontiguousarray(a)
    if a.size <= FULL_MAX:
        return a
    return np.frombuffer(hashlib.sha256(('%s%s' % (a.dtype.str, a.shape)).encode() + a.tobytes()).digest(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(H, W):
    """The one set of host inputs of a grid, shared by every case on it: read, never written."""
    rng = np.random.default_rng([33, H, W])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = {'pred': f32(rng.uniform(-1, 1, (N, H, W))), 'target': f32(rng.uniform(-1, 1, (N, H, W)))}
    d['rhs'] = f32(rng.standard_normal((N, H, W)) * 50)                         # independent of pred: the residual does not cancel
    d['rho'] = f32(rng.uniform(1.0, 10.0, (N, H, W)))
    d['dx2'] = f32(rng.uniform(5e-3, 5e-2, (N, 2)))                             # a different spacing per sample and per axis
    return d


def run(case, d):
    """One case on the GPU -> the (N, 8) float32 rows."""
    from poisson_cnn_amd import ops
    op, _, t, f = case
    dev = lambda a: torch.tensor(a, device='cuda')
    target, rhs = (dev(d['target']) if t else None), (dev(d['rhs']) if f else None)
    if op == 'error_stats':
        out = ops.error_stats(dev(d['pred']), target, rhs, dev(d['dx2']) if f else None)
    else:
        out = ops.varcoef_error_stats(dev(d['pred']), dev(d['rho']), target, rhs, dev(np.ascontiguousarray(d['dx2'][:, 0])) if f else None)
    return out.cpu().numpy()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {}
    for case in CASES:
        H, W = case[1]
        d = inputs(H, W)
        out.update({'in/%dx%d/%s' % (H, W, k): stored(v) for k, v in d.items()})
        out['out/' + case_id(case)] = run(case, d)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print('wrote %s: %d cases, %d arrays, %d bytes' % (path, len(CASES), len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
