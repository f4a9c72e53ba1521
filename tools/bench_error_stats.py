"""ops.error_stats (csrc/error_stats.hip: one pass over pred, target and rhs) at 8 x 1024^2 against the three launches that produced the nearest
figures before it existed, on the same tensors:

  ops.loss_partials(pred, target, None)      sum|e|, sum e^2, max|t|          (pcnn_loss_partials_p)
  ops.pi_loss_partials(pred, rhs, kern)      sum r^2, 3 x 3 stencil           (pcnn_pi_loss_partials_rect)
  rhs.abs().amax(dim=(1, 2))                 max|f|                           (torch, as losses.loss_wrapper normalises the residual)

- which between them still lack max|e|, sum t^2, max|r| and sum f^2.  The two routes are timed alternately, `--repeats` times each, every timing a
host clock around `--calls` back-to-back calls that end in a device synchronise; reported are the median per-call time, the spread
(max - min) / median over the repeats, and the achieved fraction of the HBM peak on the ALGORITHMIC traffic of 12 B per grid point (each of the
three fields read once).  The one-pass sums are compared with the three-launch ones (relative difference) before anything is timed.  A record,
not a gate: no threshold is applied.

    python tools/bench_error_stats.py [--calls 50] [--repeats 7] [--warmup 5] [--out profiles/error_stats.txt]

The variable-density case: `--neumann-mask M [M ...]` times ops.varcoef_error_stats(pred, rho, target, rhs, dx, neumann_mask=M)
for every mask given - mask 0 is pcnn_varcoef_error_stats, any other pcnn_varcoef_bc_error_stats - and ops.error_stats beside them, all alternated
with the same timing method, on 16 B per grid point (four fields).  Reported per route: the median, the spread and the fastest and slowest timing;
per mask its median over mask 0's.  A library of another commit (PCNN_LIBRARY) has the two old entry points only: give it `--neumann-mask 0`.

    python tools/bench_error_stats.py --neumann-mask 0 5 15 [--out profiles/varcoef_error_stats_bc.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X, the figure bench.py's roofline uses


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=50)
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--neumann-mask', type=int, nargs='+', default=None, help='the variable-density case: the masks (0..15) to time')
    p.add_argument('--out', default=None, help='default: profiles/error_stats.txt, or profiles/varcoef_error_stats_bc.txt with --neumann-mask')
    args = p.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'error_stats.txt' if args.neumann_mask is None else 'varcoef_error_stats_bc.txt')
    import torch
    from poisson_cnn_amd import _lib, ops
    N, S = args.batch, args.size
    g = torch.Generator(device='cuda').manual_seed(S)
    pred = torch.randn(N, S, S, device='cuda', generator=g)
    target = torch.randn(N, S, S, device='cuda', generator=g)
    rhs = torch.randn(N, S, S, device='cuda', generator=g) * 50
    dx = torch.rand(N, 2, device='cuda', generator=g) * 0.045 + 0.005

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls

    def alternate(routes):
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                times[k].append(timed(fn))
        return times

    def finish(lines):
        text = '\n'.join(lines) + '\n'
        print(text, end='')
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)

    if args.neumann_mask is not None:
        rho = torch.rand(N, S, S, device='cuda', generator=g) * 9.0 + 1.0
        h = dx[:, 0].contiguous()
        routes = {'error_stats (constant coefficient)': lambda: ops.error_stats(pred, target, rhs, dx)}
        for m in args.neumann_mask:
            routes['varcoef_error_stats, neumann_mask %d' % m] = (lambda m=m: ops.varcoef_error_stats(pred, rho, target, rhs, h, neumann_mask=m))
        times = alternate(routes)
        nbytes = {k: (12.0 if k.startswith('error_stats') else 16.0) * N * S * S for k in routes}
        lines = ['ops.varcoef_error_stats by Neumann mask beside ops.error_stats, %d x %d x %d float32, %s' % (N, S, S, torch.cuda.get_device_name(0)),
                 'library %s; kernel sources of this tree %s; %d calls per timing, %d timings per route (alternated), %d warm-up calls'
                 % (os.path.basename(_lib.LIB_PATH) if os.environ.get('PCNN_LIBRARY') else 'of this tree', _lib.source_hash(), args.calls, args.repeats, args.warmup),
                 'algorithmic traffic 12 B per point (error_stats) / 16 B per point (varcoef_error_stats: pred, target, rho, rhs once each); HBM peak taken as %.0f GB/s'
                 % HBM_PEAK_GBS,
                 'back-to-back calls on the same tensors: a working set below the 256 MB Infinity Cache is served from it, not from HBM', '']
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            lines.append('%-38s %8.1f us per call (median; min %.1f, max %.1f, spread %.1f %%)  %7.1f GB/s = %.1f %% of HBM peak'
                         % (k, med[k] * 1e6, min(v) * 1e6, max(v) * 1e6, 100.0 * (max(v) - min(v)) / med[k], nbytes[k] / med[k] / 1e9,
                            100.0 * nbytes[k] / med[k] / 1e9 / HBM_PEAK_GBS))
        base = 'varcoef_error_stats, neumann_mask 0'
        if base in med:
            lines += [''] + ['mask %d / mask 0: %.3f x' % (m, med['varcoef_error_stats, neumann_mask %d' % m] / med[base]) for m in args.neumann_mask if m]
        return finish(lines)

    kern = torch.zeros(N, 3, 3, device='cuda')
    ay, ax = 1.0 / dx[:, 0] ** 2, 1.0 / dx[:, 1] ** 2
    kern[:, 0, 1] = kern[:, 2, 1] = ay
    kern[:, 1, 0] = kern[:, 1, 2] = ax
    kern[:, 1, 1] = -2.0 * (ay + ax)

    def one_pass():
        return ops.error_stats(pred, target, rhs, dx)

    def three_launches():
        return ops.loss_partials(pred, target, None), ops.pi_loss_partials(pred, rhs, kern), rhs.abs().amax(dim=(1, 2))

    a = one_pass().double()
    lp, pi, _ = three_launches()
    agree = {'sum|e|': float(((a[:, 0] - lp[:, 0].double()).abs() / lp[:, 0].double()).max()),
             'sum e^2': float(((a[:, 1] - lp[:, 1].double()).abs() / lp[:, 1].double()).max()),
             'max|t|': float((a[:, 4] - lp[:, 3].double()).abs().max()),
             'sum r^2': float(((a[:, 5] - pi.double()).abs() / pi.double()).max())}

    times = alternate({'error_stats (one pass)': one_pass, 'loss_partials + pi_loss_partials + amax': three_launches})
    nbytes = 12.0 * N * S * S
    lines = ['ops.error_stats against the three-launch route, %d x %d x %d float32, %s' % (N, S, S, torch.cuda.get_device_name(0)),
             'kernel sources %s; %d calls per timing, %d timings per route (alternated), %d warm-up calls' % (_lib.source_hash(), args.calls, args.repeats, args.warmup),
             'algorithmic traffic 12 B per point = %.1f MB; HBM peak taken as %.0f GB/s' % (nbytes / 1e6, HBM_PEAK_GBS),
             'back-to-back calls on the same tensors: a working set below the 256 MB Infinity Cache is served from it, not from HBM', '']
    for k, v in times.items():
        med = statistics.median(v)
        lines.append('%-42s %8.1f us per call (median; spread %.1f %%)  %7.1f GB/s = %.1f %% of HBM peak'
                     % (k, med * 1e6, 100.0 * (max(v) - min(v)) / med, nbytes / med / 1e9, 100.0 * nbytes / med / 1e9 / HBM_PEAK_GBS))
    m = {k: statistics.median(v) for k, v in times.items()}
    ks = list(m)
    lines += ['', 'three launches / one pass: %.2f x' % (m[ks[1]] / m[ks[0]]),
              'one pass vs three launches, largest relative difference over the samples: ' + ', '.join('%s %.2g' % kv for kv in agree.items())]
    finish(lines)


if __name__ == '__main__':
    main()
