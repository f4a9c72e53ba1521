"""The Jacobi smoother (layers.JacobiIterationLayer) at 8 x 1024^2 and 32 x 512^2, n_iterations = 5 and 20:

  - the per-sweep route with the [3,3] stencil (one full-tensor launch per sweep: the default path),
  - the fused route (csrc/stencil.hip: up to ops.jacobi_k_max sweeps per launch, blocked in LDS) with [3,3], [5,5] and [9,9],

forward, as time per call and as effective GB/s on the ALGORITHMIC traffic of 12 B per grid point (read guess, read rhs, write result - what a
smoother that kept everything on chip between sweeps would move), next to the traffic model of DESIGN.md section 11:

  per-sweep  12 n B/px
  fused      sum over the launches (k sweeps each) of 4 ((T + 2 k ry)(T + 2 k rx) + (T + 2 (k-1) ry)(T + 2 (k-1) rx)) / T^2 + 4 B/px

The routes are timed alternately, `--repeats` times each, every timing a host clock around `--calls` back-to-back calls that end in a device
synchronise; the spread reported is (max - min) / median over the repeats' per-call times.  The fused [3,3] result is compared with the per-sweep
result on the same inputs (rel-L2) before anything is timed.  No threshold is applied.

    python tools/bench_jacobi.py [--calls 20] [--repeats 7] [--warmup 3] [--out profiles/jacobi_bench.json]

With `--neumann-mask M[,M...]` it measures the boundary-aware entry points instead (pcnn_jacobi_fused_bc_fwd/bwd, called through the handle so that
mask 0 runs them too) against the frozen-band ones (pcnn_jacobi_fused_fwd/bwd) in the same process: 5 sweeps, stencils [3,3] and [9,9], both shapes,
forward and adjoint, the routes alternated and timed in the same way.

    python tools/bench_jacobi.py --neumann-mask 0,15 [--out profiles/jacobi_bc_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launch_depths(n, kmax):
    """The sweeps per launch pcnn_jacobi_fused_fwd chains for n sweeps: ceil(n / kmax) launches of near-equal depth."""
    launches = -(-n // kmax)
    out, left = [], n
    for l in range(launches):
        k = -(-left // (launches - l))
        out.append(k)
        left -= k
    return out


def model_bytes_per_px(n, ss, T, kmax):
    ry, rx = ss[0] // 2, ss[1] // 2
    b = 0.0
    for k in launch_depths(n, kmax):
        b += 4.0 * ((T + 2 * k * ry) * (T + 2 * k * rx) + (T + 2 * (k - 1) * ry) * (T + 2 * (k - 1) * rx)) / float(T * T) + 4.0
    return b


def bench_bc(args, masks):
    from ctypes import c_int
    import torch
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    n = 5
    res = {'device': torch.cuda.get_device_name(0), 'n_sweeps': n, 'calls_per_timing': args.calls, 'repeats': args.repeats, 'cases': []}
    h = ops.handle()
    for (N, S) in ((8, 1024), (32, 512)):
        g = torch.Generator(device='cuda').manual_seed(S)
        u = torch.randn(N, S, S, 1, device='cuda', generator=g)
        rhs = torch.randn(N, S, S, 1, device='cuda', generator=g)
        dx2 = torch.rand(N, 2, device='cuda', generator=g) * 0.045 + 0.005
        out = torch.empty_like(u)
        dims = (c_int(N), c_int(S), c_int(S))
        for ss in ((3, 3), (9, 9)):
            coef = JacobiIterationLayer(n, ss, (2, 2), fused=True).coefficient_rows(dx2)
            sz = (c_int(ss[0]), c_int(ss[1]))
            for direction in ('fwd', 'bwd'):
                def frozen():
                    if direction == 'fwd':
                        h.call('pcnn_jacobi_fused_fwd', *dims, *sz, ops._p(coef), ops._p(u), ops._p(rhs), c_int(n), ops._p(out))
                    else:
                        h.call('pcnn_jacobi_fused_bwd', *dims, *sz, ops._p(coef), ops._p(u), c_int(n), ops._p(out))

                def aware(m):
                    if direction == 'fwd':
                        h.call('pcnn_jacobi_fused_bc_fwd', *dims, *sz, ops._p(coef), ops._p(u), ops._p(rhs), c_int(n), c_int(m), ops._p(out))
                    else:
                        h.call('pcnn_jacobi_fused_bc_bwd', *dims, *sz, ops._p(coef), ops._p(u), c_int(n), c_int(m), ops._p(out))
                routes = [('frozen', frozen)] + [('mask_%d' % m, (lambda m=m: aware(m))) for m in masks]
                for _, fn in routes:
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = [[] for _ in routes]
                for _ in range(args.repeats):
                    for i, (_, fn) in enumerate(routes):
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            fn()
                        torch.cuda.synchronize()
                        times[i].append((time.perf_counter() - t0) * 1e3 / args.calls)
                case = {'N': N, 'H': S, 'W': S, 'stencil': list(ss), 'direction': direction, 'routes': []}
                for (name, _), t in zip(routes, times):
                    t = sorted(t)
                    med = t[len(t) // 2]
                    case['routes'].append({'route': name, 'median_ms': med, 'min_ms': t[0], 'max_ms': t[-1], 'spread': (t[-1] - t[0]) / med})
                base = case['routes'][0]['median_ms']
                for r in case['routes']:
                    r['vs_frozen'] = r['median_ms'] / base
                res['cases'].append(case)
                print('%dx%dx%d %s %s n=%d: ' % (N, S, S, list(ss), direction, n) + ' | '.join('%s %.3f ms (x%.3f, spread %.1f%%)' % (r['route'], r['median_ms'],
                      r['vs_frozen'], 100 * r['spread']) for r in case['routes']), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({'jacobi_bc_bench': 'done', 'cases': len(res['cases'])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--neumann-mask', default=None, help='comma-separated masks: time the boundary-aware entry points against the frozen-band ones')
    args = ap.parse_args()
    import torch
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    if not torch.cuda.is_available():
        raise SystemExit('bench_jacobi.py measures on the GPU; none found')
    if args.neumann_mask is not None:
        return bench_bc(args, [int(m, 0) for m in args.neumann_mask.split(',')])
    T = ops.jacobi_tile()
    res = {'device': torch.cuda.get_device_name(0), 'tile': T, 'algorithmic_bytes_per_px': 12, 'calls_per_timing': args.calls, 'repeats': args.repeats, 'cases': []}
    for (N, S) in ((8, 1024), (32, 512)):
        g = torch.Generator(device='cuda').manual_seed(S)
        u = torch.randn(N, S, S, 1, device='cuda', generator=g)
        rhs = torch.randn(N, S, S, 1, device='cuda', generator=g)
        dx2 = torch.rand(N, 2, device='cuda', generator=g) * 0.045 + 0.005
        px = N * S * S
        for n in (5, 20):
            routes = [('per_sweep', (3, 3), JacobiIterationLayer(n))]
            routes += [('fused', ss, JacobiIterationLayer(n, ss, (2, 2), fused=True)) for ss in ((3, 3), (5, 5), (9, 9))]
            y_ps = routes[0][2].forward(u, rhs, dx2)
            y_f = routes[1][2].forward(u, rhs, dx2)
            agree = float((y_f - y_ps).double().norm() / y_ps.double().norm())
            for _, _, lay in routes:
                for _ in range(args.warmup):
                    lay.forward(u, rhs, dx2)
            torch.cuda.synchronize()
            times = [[] for _ in routes]
            for _ in range(args.repeats):                      # alternate the routes: drift of the shared host / clocks hits all of them alike
                for i, (_, _, lay) in enumerate(routes):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        lay.forward(u, rhs, dx2)
                    torch.cuda.synchronize()
                    times[i].append((time.perf_counter() - t0) * 1e3 / args.calls)
            case = {'N': N, 'H': S, 'W': S, 'n_iterations': n, 'fused_3x3_vs_per_sweep_rel_l2': agree, 'routes': []}
            for (name, ss, lay), t in zip(routes, times):
                t = sorted(t)
                med = t[len(t) // 2]
                kmax = ops.jacobi_k_max(*ss)
                model = 12.0 * n if name == 'per_sweep' else model_bytes_per_px(n, ss, T, kmax)
                case['routes'].append({'route': name, 'stencil': list(ss), 'launches': n if name == 'per_sweep' else len(launch_depths(n, kmax)),
                                       'median_ms': med, 'min_ms': t[0], 'max_ms': t[-1], 'spread': (t[-1] - t[0]) / med,
                                       'effective_GBps_on_12B_per_px': 12.0 * px / (med * 1e-3) / 1e9, 'model_bytes_per_px': model,
                                       'model_GBps_moved': model * px / (med * 1e-3) / 1e9})
            ps, f3 = case['routes'][0], case['routes'][1]
            case['fused_3x3_speedup_measured'] = ps['median_ms'] / f3['median_ms']
            case['fused_3x3_speedup_traffic_model'] = ps['model_bytes_per_px'] / f3['model_bytes_per_px']
            res['cases'].append(case)
            print('%dx%dx%d n=%d: ' % (N, S, S, n) + ' | '.join('%s %s %.3f ms (%.0f GB/s eff, spread %.1f%%)' % (r['route'], r['stencil'], r['median_ms'],
                  r['effective_GBps_on_12B_per_px'], 100 * r['spread']) for r in case['routes'])
                  + ' | fused [3,3] vs per-sweep: %.2fx measured, %.2fx traffic model, rel-L2 %.1e'
                  % (case['fused_3x3_speedup_measured'], case['fused_3x3_speedup_traffic_model'], agree), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({'jacobi_bench': 'done', 'cases': len(res['cases'])}))


if __name__ == '__main__':
    main()
