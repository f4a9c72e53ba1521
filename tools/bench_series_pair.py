"""pcnn_series_pair_synthesis (csrc/dataset.hip: series_pair_kernel, one launch for a solution / right-hand side pair) against the two
pcnn_series_synthesis launches the sine and cosine generators spend on the same pair (`coef`, then `coef * adj`), on the same coefficients and
sine bases, at two shapes:

  50 x 384 x 384, 8 x 8 modes      the largest batch the shipped training workload generates (experiments/hpnn.json: batch 50, grids up to 384,
                                   fourier_coeff_grid_size_range up to 8)
  8 x 1024 x 1024, 8 x 8 modes     a large grid

Every entry point is called through the C ABI on preallocated outputs, so no allocation is timed.  The two routes are timed alternately,
`--repeats` times each; every timing is a pair of device events around `--calls` back-to-back calls.  Reported per route and shape: the median
per-pair time, the spread (max - min) / median over the repeats, and the achieved fraction of the HBM peak on the ALGORITHMIC traffic of 8 B per
grid point (both fields written once; the tables read are a few hundred bytes).  The two routes' outputs are compared (rel-L2) before anything
is timed.  A record, not a gate: no threshold is applied.

    python tools/bench_series_pair.py [--calls 50] [--repeats 7] [--warmup 5] [--out profiles/series_pair.txt]
"""
import argparse
import math
import os
import statistics
import sys
from ctypes import c_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X, the figure bench.py's roofline uses
SHAPES = ((50, 384, 384, 8, 8), (8, 1024, 1024, 8, 8))


def bench_shape(args, N, H, W, ka, kb):
    import numpy as np
    import torch
    from poisson_cnn_amd.ops import _p, handle
    rng = np.random.default_rng(H)
    coef = 2 * rng.uniform(size=(N, ka, kb)) - 1
    L = rng.uniform(5e-3, 5e-2, (N, 1)) * np.array([H, W], dtype=np.float64)[None]
    lam_a = -(math.pi * np.arange(1, ka + 1)[None, :] / L[:, 0, None]) ** 2
    lam_b = -(math.pi * np.arange(1, kb + 1)[None, :] / L[:, 1, None]) ** 2
    adj = lam_a[:, :, None] + lam_b[:, None, :]
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda')
    c, ca, la, lb = dev(coef), dev(coef * adj), dev(lam_a), dev(lam_b)
    u1, f1, u2, f2 = (torch.empty(N, H, W, device='cuda') for _ in range(4))
    h = handle()
    dims = (c_int(N), c_int(H), c_int(W), c_int(ka), c_int(kb))

    def pair():
        h.call('pcnn_series_pair_synthesis', *dims, _p(c), _p(la), _p(lb), c_int(0), c_int(0), _p(u1), _p(f1))

    def two_launches():
        h.call('pcnn_series_synthesis', *dims, _p(c), c_int(0), c_int(0), _p(u2))
        h.call('pcnn_series_synthesis', *dims, _p(ca), c_int(0), c_int(0), _p(f2))

    pair()
    two_launches()
    torch.cuda.synchronize()
    agree = (float((u1.double() - u2.double()).norm() / u2.double().norm()), float((f1.double() - f2.double()).norm() / f2.double().norm()))

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3 / args.calls

    routes = {'series_pair_synthesis (one launch)': pair, 'series_synthesis x 2 (coef, coef * adj)': two_launches}
    for fn in routes.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in routes}
    for _ in range(args.repeats):
        for k, fn in routes.items():
            times[k].append(timed(fn))
    nbytes = 8.0 * N * H * W
    lines = ['%d x %d x %d, %d x %d modes: 8 B per point = %.1f MB written per pair' % (N, H, W, ka, kb, nbytes / 1e6)]
    for k, v in times.items():
        med = statistics.median(v)
        lines.append('  %-42s %8.1f us per pair (median; spread %.1f %%)  %7.1f GB/s = %.1f %% of HBM peak'
                     % (k, med * 1e6, 100.0 * (max(v) - min(v)) / med, nbytes / med / 1e9, 100.0 * nbytes / med / 1e9 / HBM_PEAK_GBS))
    m = [statistics.median(v) for v in times.values()]
    lines += ['  two launches / one launch: %.2f x' % (m[1] / m[0]),
              '  one launch vs two launches, rel-L2: soln %.2g, rhs %.2g' % agree, '']
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=50)
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'series_pair.txt'))
    args = p.parse_args(argv)
    import torch
    from poisson_cnn_amd import _lib
    lines = ['pcnn_series_pair_synthesis against two pcnn_series_synthesis launches, float32, %s' % torch.cuda.get_device_name(0),
             'kernel sources %s; %d calls per timing (device events), %d timings per route (alternated), %d warm-up calls'
             % (_lib.source_hash(), args.calls, args.repeats, args.warmup),
             'HBM peak taken as %.0f GB/s; back-to-back calls on the same tensors: a working set below the 256 MB Infinity Cache is served from it, not from HBM'
             % HBM_PEAK_GBS, '']
    for shape in SHAPES:
        lines += bench_shape(args, *shape)
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
