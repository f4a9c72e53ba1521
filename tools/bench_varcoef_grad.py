"""The gather kernels of the differentiable variable-density solve (csrc/varcoef_grad.hip) against a copy of the same bytes,
and the whole backward of autograd.variable_density_solve against a cold forward solve.

  8 x 512 x 512 and 8 x 1024 x 1024, neumann_mask 0 and 9:
    pcnn_varcoef_bc_coef_grad (reads u, lam, rho, writes drho: 16 B per point) and pcnn_varcoef_bc_pi_loss_bwd_inputs (reads pred, rho, rhs, writes
    drhs, drho: 20 B per point) through the C ABI on preallocated outputs, against torch's device-to-device copy (float4 loads and stores) of a
    float32 buffer that moves the same bytes (half read, half written);
    loss.backward() through autograd.variable_density_solve (the adjoint solve, coef_grad, edge_grad) against the forward solve, cold start.

Every timing is a pair of device events around `--calls` back-to-back launches (kernels) or one call (solves), `--repeats` times, the routes of one
shape alternated; reported: the median and the spread (max - min) / median.  A record, not a gate: no threshold.

    python tools/bench_varcoef_grad.py [--calls 20] [--repeats 9] [--warmup 2] [--out profiles/varcoef_grad.txt]
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
SHAPES = ((8, 512, 512), (8, 1024, 1024))
MASKS = (0, 9)


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


def summary(name, v, extra=''):
    med = statistics.median(v)
    return '  %-52s %9.3f ms (median of %d; spread %.1f %%)%s' % (name, med * 1e3, len(v), 100.0 * (max(v) - min(v)) / med, extra)


def fields(N, H, W, seed):
    import numpy as np
    import torch
    from poisson_cnn_amd.dataset import _kernels as K
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device='cuda').contiguous()
    x, y = np.linspace(0, 1, H)[None, :, None], np.linspace(0, 1, W)[None, None, :]
    rho = K.varcoef_density_smooth(dev(np.cos(3 * np.pi * x + rng.uniform(size=(N, 1, 1))) * np.cos(2 * np.pi * y)), 1.0, 10.0)
    return rho, dev(rng.standard_normal((N, H, W))), dev(rng.standard_normal((N, H, W))), dev(np.full((N,), 1.0 / (W - 1)))


def bench_kernels(args, N, H, W):
    import torch
    from poisson_cnn_amd.ops import _p, handle
    rho, u, lam, dx = fields(N, H, W, H)
    coef = torch.ones(N, device='cuda')
    drho, drhs = torch.empty_like(rho), torch.empty_like(rho)
    h = handle()
    lines = ['%d x %d x %d: the gather kernels alone' % (N, H, W)]
    for mask in MASKS:
        routes = {
            'coef_grad, mask %d (16 B per point)' % mask: (16, lambda: h.call('pcnn_varcoef_bc_coef_grad', c_int(N), c_int(H), c_int(W), c_int(mask), _p(rho), _p(dx), _p(u), _p(lam), _p(None), _p(None), _p(None), _p(None), _p(drho))),
            'pi_loss_bwd_inputs, mask %d (20 B per point)' % mask: (20, lambda: h.call('pcnn_varcoef_bc_pi_loss_bwd_inputs', c_int(N), c_int(H), c_int(W), _p(u), _p(rho), _p(lam), _p(dx), _p(coef), _p(drhs), _p(drho), c_int(mask))),
        }
        for per in (16, 20):
            src = torch.empty(N * H * W * per // 8, device='cuda')
            dst = torch.empty_like(src)
            routes['copy of %d B per point' % per] = (per, lambda s=src, d=dst: d.copy_(s))
        for _, fn in routes.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, (_, fn) in routes.items():
                times[k].append(event_time(fn, args.calls))
        for k, (per, _) in routes.items():
            gbs = per * N * H * W / statistics.median(times[k]) / 1e9
            lines.append(summary(k, times[k], '  %7.1f GB/s = %.1f %% of HBM peak' % (gbs, 100.0 * gbs / HBM_PEAK_GBS)))
    return lines + ['']


def bench_backward(args, N, H, W):
    import torch
    from poisson_cnn_amd import autograd
    rho, rhs, wts, dx = fields(N, H, W, W)
    edges = {k: torch.zeros(N, W if k in ('left', 'right') else H, device='cuda') for k in ('left', 'right', 'bottom', 'top')}
    lines = ['%d x %d x %d: autograd.variable_density_solve, tol 1e-10, preconditioner dst, gradients w.r.t. rho, rhs and the four edges' % (N, H, W)]
    for mask in MASKS:
        types = {k: ('neumann' if mask >> i & 1 else 'dirichlet') for i, k in enumerate(('left', 'right', 'bottom', 'top'))}
        leaves = [rho.clone().requires_grad_(True), rhs.clone().requires_grad_(True)] + [v.clone().requires_grad_(True) for v in edges.values()]
        state = {}

        def forward():
            state['u'] = autograd.variable_density_solve(leaves[0], leaves[1], dict(zip(edges, leaves[2:])), dx, boundary_types=types)

        def backward():
            for t in leaves:
                t.grad = None
            (state['u'][:, 0] * wts).sum().backward()
        fwd, bwd = [], []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            for i in range(args.warmup + args.repeats):
                tf = event_time(forward)
                tb = event_time(backward)
                if i >= args.warmup:
                    fwd.append(tf)
                    bwd.append(tb)
        lines += [summary('forward solve, mask %d' % mask, fwd), summary('backward (adjoint solve + gathers), mask %d' % mask, bwd),
                  '  backward / forward: %.2f' % (statistics.median(bwd) / statistics.median(fwd))]
    return lines + ['']


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--repeats', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_grad.txt'))
    args = p.parse_args(argv)
    import torch
    from poisson_cnn_amd import _lib
    lines = ['Gradients of the variable-density problem w.r.t. its data, float32 fields, %s' % torch.cuda.get_device_name(0),
             'kernel sources %s; device events; %d timings per route (alternated), %d warm-up calls; kernels: %d launches per timing'
             % (_lib.source_hash(), args.repeats, args.warmup, args.calls),
             'HBM peak taken as %.0f GB/s; back-to-back launches on the same tensors: a working set below the 256 MB Infinity Cache is served from it' % HBM_PEAK_GBS, '']
    for shape in SHAPES:
        lines += bench_kernels(args, *shape)
    for shape in SHAPES:
        lines += bench_backward(args, *shape)
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
