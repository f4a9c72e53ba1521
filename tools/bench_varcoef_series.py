"""The solve-free variable-density generator (dataset.reverse_variable_density_dataset_generator: one pcnn_varcoef_series_pair launch per batch,
DESIGN.md section 23) against the solver-made one (dataset.variable_density_dataset_generator, preconditioner 'dst', density_profile 'abs'), and
the kernel alone.

  one __getitem__ of each generator at 16 x 512 x 512 and 50 x 384 x 384, density ratio 10 and 1000 (the series generator with 8 x 8 modes at most)
  pcnn_varcoef_series_pair alone at 8 x 1024 x 1024 with 8 x 8 and 16 x 16 modes, through the C ABI on preallocated outputs

Every timing is a pair of device events; a generator timing spans one whole __getitem__ (host draws, uploads, launches; the solver's flag reads
included) and ends in the stop event's synchronise, a kernel timing spans `--calls` back-to-back launches.  The routes of one shape are timed
alternately, `--repeats` times each; reported: the median, the spread (max - min) / median, grids per second, and for the kernel the achieved
bytes per second on the ALGORITHMIC traffic of 12 B per grid point (rho read once, soln and rhs written once).  A record, not a gate: no threshold.

    python tools/bench_varcoef_series.py [--calls 20] [--repeats 9] [--warmup 2] [--out profiles/varcoef_series.txt]
"""
import argparse
import os
import statistics
import sys
import warnings
from ctypes import c_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X, the figure bench.py's roofline uses
GENERATOR_SHAPES = ((16, 512, 512), (50, 384, 384))
RATIOS = (10.0, 1000.0)
KERNEL_SHAPES = ((8, 1024, 1024, 8, 8), (8, 1024, 1024, 16, 16))


def event_time(fn, calls=1):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / calls


def summary(name, v, grids, extra=''):
    med = statistics.median(v)
    return '  %-44s %9.3f ms (median of %d; spread %.1f %%)  %8.1f grids/s%s' % (name, med * 1e3, len(v), 100.0 * (max(v) - min(v)) / med, grids / med, extra)


def bench_generators(args, N, H, W, ratio):
    from poisson_cnn_amd import dataset as D
    common = dict(batch_size=N, batches_per_epoch=1, output_shape=(H, W), density_range=(1.0, ratio), density_profile='abs', seed=3)
    series = D.reverse_variable_density_dataset_generator(fourier_coeff_grid_size_range=(1, 8), **common)
    solver = D.variable_density_dataset_generator(preconditioner='dst', **common)
    routes = {'reverse_variable_density_dataset_generator': lambda: series[0], 'variable_density_dataset_generator (dst)': lambda: solver[0]}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # a sample that runs out of iterations is reported below, not on stderr
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        times, iters = {k: [] for k in routes}, []
        for _ in range(args.repeats):
            for k, fn in routes.items():
                times[k].append(event_time(fn))
            iters.append((int(solver.last_info['iterations'].max()), bool(solver.last_info['converged'].all())))
    lines = ['%d x %d x %d, density ratio %g: one __getitem__' % (N, H, W, ratio)]
    lines += [summary(k, v, N) for k, v in times.items()]
    m = [statistics.median(v) for v in times.values()]
    lines += ['  solver-made / solve-free: %.1f x;  solver iterations per batch (largest sample) %d..%d, all converged: %s'
              % (m[1] / m[0], min(i for i, _ in iters), max(i for i, _ in iters), all(c for _, c in iters)), '']
    return lines


def bench_kernel(args, N, H, W, ka, kb):
    import numpy as np
    import torch
    from poisson_cnn_amd.dataset import _kernels as K
    from poisson_cnn_amd.ops import _p, handle
    rng = np.random.default_rng(H + ka)
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda').contiguous()
    coef, dx = dev(2 * rng.uniform(size=(N, ka, kb)) - 1), dev(rng.uniform(5e-3, 5e-2, (N,)))
    x, y = np.linspace(0, 1, H)[None, :, None], np.linspace(0, 1, W)[None, None, :]
    rho = K.varcoef_density(dev(np.cos(3 * np.pi * x + rng.uniform(size=(N, 1, 1))) * np.cos(2 * np.pi * y)), 1.0, 1000.0)
    soln, rhs = torch.empty(N, H, W, device='cuda'), torch.empty(N, H, W, device='cuda')
    h = handle()
    lines = ['%d x %d x %d, %d x %d modes: pcnn_varcoef_series_pair alone, 12 B per point = %.1f MB per launch' % (N, H, W, ka, kb, 12.0 * N * H * W / 1e6)]
    for mask in (0, 15):
        fn = lambda: h.call('pcnn_varcoef_series_pair', c_int(N), c_int(H), c_int(W), c_int(ka), c_int(kb), _p(coef), c_int(mask), _p(rho), _p(dx), _p(soln), _p(rhs))
        for _ in range(args.warmup):
            fn()
        v = [event_time(fn, args.calls) for _ in range(args.repeats)]
        gbs = 12.0 * N * H * W / statistics.median(v) / 1e9
        lines.append(summary('neumann_mask %d' % mask, v, N, '  %7.1f GB/s = %.1f %% of HBM peak' % (gbs, 100.0 * gbs / HBM_PEAK_GBS)))
    return lines + ['']


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--repeats', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_series.txt'))
    args = p.parse_args(argv)
    import torch
    from poisson_cnn_amd import _lib
    lines = ['Solve-free against solver-made variable-density training data, float32 fields, %s' % torch.cuda.get_device_name(0),
             'kernel sources %s; device events; %d timings per route (alternated), %d warm-up calls; kernel alone: %d launches per timing'
             % (_lib.source_hash(), args.repeats, args.warmup, args.calls),
             'HBM peak taken as %.0f GB/s; back-to-back launches on the same tensors: a working set below the 256 MB Infinity Cache is served from it' % HBM_PEAK_GBS, '']
    for shape in GENERATOR_SHAPES:
        for ratio in RATIOS:
            lines += bench_generators(args, *shape, ratio)
    for shape in KERNEL_SHAPES:
        lines += bench_kernel(args, *shape)
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
