"""The backward of the variable-density smoother with respect to all its inputs (pcnn_varcoef_bc_jacobi_bwd_inputs of csrc/varcoef_train.hip,
DESIGN.md section 25) against the adjoint w.r.t. u alone on the same inputs and against a copy of the same bytes.

  8 x 512 x 512 and 8 x 1024 x 1024, 5 sweeps, neumann_mask 0 and 9, through the C ABI on preallocated outputs:
    bwd_inputs (du, drho, drhs): per point the recomputation reads rho, u, rhs and writes an iterate per sweep (16 B x n), and each backward sweep
      reads rho, two iterates and a gradient, writes a gradient (20 B x n) and reads and writes drho and drhs (16 B, 8 B in the first) -
      52 n - 8 = 252 B per point for n = 5;
    bwd_inputs (drho, drhs): the same without the last gradient write;
    jacobi_bwd (du alone, ops.varcoef_jacobi_bwd): the n sweeps fused in one launch, 12 B per point;
    torch's device-to-device copy (float4 loads and stores) of a float32 buffer that moves 252 B per point (half read, half written).

Every timing is a pair of device events around `--calls` back-to-back calls, `--repeats` times, the routes of one shape alternated; reported: the
median and the spread (max - min) / median.  A record, not a gate: no threshold.

    python tools/bench_varcoef_jacobi_grad.py [--calls 10] [--repeats 9] [--warmup 2] [--out profiles/varcoef_jacobi_grad.txt]
"""
import argparse
import os
import statistics
import sys
from ctypes import c_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_varcoef_grad import HBM_PEAK_GBS, event_time, fields, summary      # noqa: E402  (the method of that record)

SHAPES = ((8, 512, 512), (8, 1024, 1024))
MASKS = (0, 9)
SWEEPS = 5


def bytes_per_point(n, with_du=True):
    return 52 * n - 8 - (0 if with_du else 4)


def bench(args, N, H, W):
    import torch
    from poisson_cnn_amd.ops import _p, handle
    rho, u, rhs, dx = fields(N, H, W, H)
    g = torch.randn_like(u)
    du, drho, drhs = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
    h = handle()
    dims = (c_int(N), c_int(H), c_int(W))
    per = bytes_per_point(SWEEPS)
    src = torch.empty(N * H * W * per // 8, device='cuda')
    dst = torch.empty_like(src)
    lines = ['%d x %d x %d, %d sweeps' % (N, H, W, SWEEPS)]
    for mask in MASKS:
        inputs = lambda a, b, c, m=mask: h.call('pcnn_varcoef_bc_jacobi_bwd_inputs', *dims, c_int(m), _p(rho), _p(u), _p(rhs), _p(dx), _p(g), c_int(SWEEPS),
                                                _p(a), _p(b), _p(c))
        routes = {
            'bwd_inputs du, drho, drhs, mask %d (%d B per point)' % (mask, per): (per, lambda: inputs(du, drho, drhs)),
            'bwd_inputs drho, drhs, mask %d (%d B per point)' % (mask, per - 4): (per - 4, lambda: inputs(None, drho, drhs)),
            'jacobi_bwd du alone, mask %d (12 B per point)' % mask: (12, lambda m=mask: h.call('pcnn_varcoef_bc_jacobi_bwd', *dims, _p(rho), _p(dx), _p(g), c_int(SWEEPS), _p(du), c_int(m))),
            'copy of %d B per point' % per: (per, lambda: dst.copy_(src)),
        }
        for _, fn in routes.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, (_, fn) in routes.items():
                times[k].append(event_time(fn, args.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (b, _) in routes.items():
            gbs = b * N * H * W / med[k] / 1e9
            lines.append(summary(k, times[k], '  %7.1f GB/s = %.1f %% of HBM peak' % (gbs, 100.0 * gbs / HBM_PEAK_GBS)))
        full, alone, copy = (med[k] for k in list(routes)[:1] + list(routes)[2:])
        lines.append('  bwd_inputs (all three) / jacobi_bwd: %.2f;  / the copy of its bytes: %.2f' % (full / alone, full / copy))
    return lines + ['']


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=10)
    p.add_argument('--repeats', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_jacobi_grad.txt'))
    args = p.parse_args(argv)
    import torch
    from poisson_cnn_amd import _lib
    lines = ['The variable-density smoother\'s backward w.r.t. u, rho and rhs, float32 fields, %s' % torch.cuda.get_device_name(0),
             'kernel sources %s; device events; %d timings per route (alternated), %d warm-up calls; %d calls per timing'
             % (_lib.source_hash(), args.repeats, args.warmup, args.calls),
             'HBM peak taken as %.0f GB/s; back-to-back calls on the same tensors: a working set below the 256 MB Infinity Cache is served from it' % HBM_PEAK_GBS, '']
    for shape in SHAPES:
        lines += bench(args, *shape)
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
