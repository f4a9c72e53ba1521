"""The four kernels of csrc/varcoef_train.hip beside their constant-coefficient siblings, at 256^2, 512^2 and 1024^2 with
the batch chosen so that every case has 8 x 1024^2 points:

  pcnn_varcoef_pi_loss_partials   vs  pcnn_pi_loss_partials_rect (3 x 3 stencil)
  pcnn_varcoef_pi_loss_bwd        vs  pcnn_pi_loss_bwd_rect      (3 x 3 stencil)
  pcnn_varcoef_jacobi_fwd         vs  pcnn_jacobi_fused_fwd      (3 x 3 stencil, the same sweep count)
  pcnn_varcoef_jacobi_bwd         vs  pcnn_jacobi_fused_bwd

Every timing is a pair of HIP events around `--calls` back-to-back calls; a kernel and its sibling alternate, `--repeats` times each, and the
median per-call time is reported with the spread (max - min) / median.  Beside each time: the bytes per point of the traffic model below, the rate
that model implies, and that rate over 0.79 x the HBM peak (the copy figure of DESIGN.md section 4).  One field of a case is 33.5 MB, so a case's
whole working set fits the 256 MB Infinity Cache: the rates say how fast the kernel streams, not that HBM delivered them.  No threshold is applied.

Traffic model (B per grid point; T x U the tile, halo reads counted, 4-byte fields):
  loss sums     pred and rho on (16+2)(64+2) per 16 x 64 tile, rhs once                          sibling: pred and rhs once (it reads the halo from cache)
  loss gradient pred and rho on (16+4)(64+4), rhs on (16+2)(64+2), dpred read and written        sibling: pred, rhs, dpred read and written
  sweeps, per launch of k: u and rho on (64+2k)^2, rhs on (64+2(k-1))^2 per 64^2 tile, one write  sibling: the same without rho
  adjoint, per launch of k: dout on (64+2k)^2, rho on (64+2k+2)^2, one write                     sibling: the same without rho

    python tools/bench_varcoef_train.py [--calls 20] [--repeats 7] [--warmup 3] [--out profiles/varcoef_train_bench.json (the default)]

--neumann-mask 0,5,15 measures something else with the same cases and protocol, and writes no JSON: the four kernels through
the all-Dirichlet entry points (mask 0) and, alternating with them, through the pcnn_varcoef_bc_* entry points for every non-zero mask of the
list; one line per case with each route's median, minimum and maximum per-call time and the ratio of the medians to mask 0.  `--neumann-mask 0` times
the old entry points alone (with PCNN_LIBRARY naming another build of the library: the same figures for that build).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X
COPY_FRACTION = 0.79


def launch_depths(n, kmax):
    launches = -(-n // kmax)
    out, left = [], n
    for l in range(launches):
        k = -(-left // (launches - l))
        out.append(k)
        left -= k
    return out


def model_bytes(kind, varcoef, n=0, kmax=8, T=64):
    rho = 1.0 if varcoef else 0.0
    if kind == 'pi_partials':
        return 4.0 * (18 * 66) / (16 * 64) * (1 + rho) + 4.0 if varcoef else 8.0
    if kind == 'pi_bwd':
        return 4.0 * (20 * 68) / (16 * 64) * 2 + 4.0 * (18 * 66) / (16 * 64) + 8.0 if varcoef else 16.0
    b = 0.0
    for k in launch_depths(n, kmax):
        if kind == 'jacobi_fwd':
            b += 4.0 * ((1 + rho) * (T + 2 * k) ** 2 + (T + 2 * (k - 1)) ** 2) / float(T * T) + 4.0
        else:
            b += 4.0 * ((T + 2 * k) ** 2 + rho * (T + 2 * k + 2) ** 2) / float(T * T) + 4.0
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_train_bench.json'))
    ap.add_argument('--neumann-mask', default=None, help='comma list of masks 0..15: time the kernels per mask instead of beside their siblings')
    args = ap.parse_args()
    masks = None
    if args.neumann_mask is not None:
        masks = sorted({int(m) for m in args.neumann_mask.split(',')})
        if not masks or masks[0] < 0 or masks[-1] > 15:
            raise SystemExit('--neumann-mask takes masks in 0..15, got %r' % args.neumann_mask)
    from ctypes import c_int
    import torch
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.layers import JacobiIterationLayer
    if not torch.cuda.is_available():
        raise SystemExit('bench_varcoef_train.py measures on the GPU; none found')
    h, p = ops.handle(), ops._p
    kmax = ops.varcoef_jacobi_k_max()
    assert kmax == ops.jacobi_k_max(3, 3) and ops.jacobi_tile() == 64
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_timing': args.calls, 'repeats': args.repeats, 'hbm_peak_GBps': HBM_PEAK_GBPS,
           'copy_fraction': COPY_FRACTION, 'k_max': kmax, 'cases': []}
    for (N, S) in ((128, 256), (32, 512), (8, 1024)):
        g = torch.Generator(device='cuda').manual_seed(S)
        u, rhs, gr = (torch.randn(N, S, S, device='cuda', generator=g) for _ in range(3))
        rho = torch.rand(N, S, S, device='cuda', generator=g) * 9 + 1
        dx = torch.rand(N, device='cuda', generator=g) * 0.045 + 0.005
        dx2 = torch.stack([dx, dx], 1).contiguous()
        coef = torch.full((N,), 1e-8, device='cuda')
        lap = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], device='cuda')
        kern = (lap[None] / dx[:, None, None] ** 2).contiguous()
        out, sums, dpred = torch.empty_like(u), torch.empty(N, device='cuda'), torch.zeros_like(u)
        dims = (c_int(N), c_int(S), c_int(S))
        px = N * S * S
        pairs = [('pi_partials', 0,
                  lambda: h.call('pcnn_varcoef_pi_loss_partials', *dims, p(u), p(rho), p(rhs), p(dx), p(sums)),
                  lambda: h.call('pcnn_pi_loss_partials_rect', *dims, c_int(3), c_int(3), p(u), p(rhs), p(kern), p(sums))),
                 ('pi_bwd', 0,
                  lambda: h.call('pcnn_varcoef_pi_loss_bwd', *dims, p(u), p(rho), p(rhs), p(dx), p(coef), p(dpred)),
                  lambda: h.call('pcnn_pi_loss_bwd_rect', *dims, c_int(3), c_int(3), p(u), p(rhs), p(kern), p(coef), p(dpred)))]
        for n in (5, kmax):
            rows = JacobiIterationLayer(n, fused=True).coefficient_rows(dx2)
            pairs.append(('jacobi_fwd', n,
                          lambda n=n: h.call('pcnn_varcoef_jacobi_fwd', *dims, p(rho), p(u), p(rhs), p(dx), c_int(n), p(out)),
                          lambda n=n, rows=rows: h.call('pcnn_jacobi_fused_fwd', *dims, c_int(3), c_int(3), p(rows), p(u), p(rhs), c_int(n), p(out))))
            pairs.append(('jacobi_bwd', n,
                          lambda n=n: h.call('pcnn_varcoef_jacobi_bwd', *dims, p(rho), p(dx), p(gr), c_int(n), p(out)),
                          lambda n=n, rows=rows: h.call('pcnn_jacobi_fused_bwd', *dims, c_int(3), c_int(3), p(rows), p(gr), c_int(n), p(out))))
        if masks is not None:
            bc = lambda m: c_int(m)
            for kind, n, mine, _ in pairs:
                routes = [('mask 0', mine)]
                for m in (m for m in masks if m):
                    if kind == 'pi_partials':
                        fn = lambda m=m: h.call('pcnn_varcoef_bc_pi_loss_partials', *dims, p(u), p(rho), p(rhs), p(dx), p(sums), bc(m))
                    elif kind == 'pi_bwd':
                        fn = lambda m=m: h.call('pcnn_varcoef_bc_pi_loss_bwd', *dims, p(u), p(rho), p(rhs), p(dx), p(coef), p(dpred), bc(m))
                    elif kind == 'jacobi_fwd':
                        fn = lambda m=m, n=n: h.call('pcnn_varcoef_bc_jacobi_fwd', *dims, p(rho), p(u), p(rhs), p(dx), c_int(n), p(out), bc(m))
                    else:
                        fn = lambda m=m, n=n: h.call('pcnn_varcoef_bc_jacobi_bwd', *dims, p(rho), p(dx), p(gr), c_int(n), p(out), bc(m))
                    routes.append(('mask %d' % m, fn))
                for _, fn in routes:
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = [[] for _ in routes]
                for _ in range(args.repeats):
                    for i, (_, fn) in enumerate(routes):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.calls):
                            fn()
                        e1.record()
                        e1.synchronize()
                        times[i].append(e0.elapsed_time(e1) / args.calls)
                times = [sorted(t) for t in times]
                base = times[0][len(times[0]) // 2]
                print('%-11s %4dx%4dx%4d n=%d: ' % (kind, N, S, S, n) + ' | '.join('%s %.4f ms (min %.4f, max %.4f)%s' % (
                    name, t[len(t) // 2], t[0], t[-1], '' if i == 0 else ' x%.3f' % (t[len(t) // 2] / base)) for i, ((name, _), t) in enumerate(zip(routes, times))),
                    flush=True)
            continue
        for kind, n, mine, sibling in pairs:
            routes = [('varcoef', mine), ('sibling', sibling)]
            for _, fn in routes:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = [[], []]
            for _ in range(args.repeats):
                for i, (_, fn) in enumerate(routes):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.calls):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[i].append(e0.elapsed_time(e1) / args.calls)
            case = {'kernel': kind, 'N': N, 'H': S, 'W': S, 'n_sweeps': n, 'routes': []}
            for (name, _), t in zip(routes, times):
                t = sorted(t)
                med = t[len(t) // 2]
                b = model_bytes(kind, name == 'varcoef', n, kmax)
                rate = b * px / (med * 1e-3) / 1e9
                case['routes'].append({'route': name, 'median_ms': med, 'min_ms': t[0], 'max_ms': t[-1], 'spread': (t[-1] - t[0]) / med, 'model_bytes_per_px': b,
                                       'model_GBps': rate, 'of_copy_rate': rate / (COPY_FRACTION * HBM_PEAK_GBPS)})
            case['varcoef_over_sibling'] = case['routes'][0]['median_ms'] / case['routes'][1]['median_ms']
            res['cases'].append(case)
            print('%-11s %4dx%4dx%4d n=%d: ' % (kind, N, S, S, n) + ' | '.join('%s %.3f ms (%.1f B/px, %.0f GB/s = %.2f of copy, spread %.1f%%)' % (
                r['route'], r['median_ms'], r['model_bytes_per_px'], r['model_GBps'], r['of_copy_rate'], 100 * r['spread']) for r in case['routes'])
                + ' | ratio %.2f' % case['varcoef_over_sibling'], flush=True)
    if args.out and masks is None:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({'varcoef_train_bench': 'done', 'cases': len(res['cases'])}))


if __name__ == '__main__':
    main()
