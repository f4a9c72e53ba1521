"""Times the variable-density Poisson solve (csrc/varcoef.hip) at 256^2, 512^2 and 1024^2: the operator launch (q = A p with
its p.q), one iteration of the preconditioned conjugate-gradient loop (from a call of pcnn_varcoef_pcg_iterate that runs 8), a whole solve at density
ratio 10 and tol = 1e-10, and - as the reference point - one fd_poisson_dst solve of the same shape.  HIP-event medians after a warm-up call.
Per-iteration bytes are reported against the traffic model of the design section (172 B per point and iteration) and the four fp64 GEMMs of the
preconditioner as FLOP/s.  Writes profiles/varcoef_bench.json.
--preconditioner scaled times the *_scaled entry points (24 B more per point and iteration), --density-profile smooth takes the
generator's smooth profile, --ratio another density ratio; with any of them set, name the file to write with --out (default: none)."""
import argparse
import json
import os
import sys
from ctypes import c_double, c_int, c_size_t

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from poisson_cnn_amd import _lib, dataset as D
from poisson_cnn_amd.dataset import _kernels as K
from poisson_cnn_amd.ops import _p, handle

MODEL_BYTES = {'apply (p, rho, q)': 20, 'x, r update (x, p, r, q -> x, r)': 48, 'four GEMMs (in, out)': 64, 'eigenvalue division': 16, 'p update (z, p -> p)': 24}
SCALED_BYTES = {'x, r update (x, p, r, q -> x, r)': 64, 'p update (z, p -> p)': 32}       # s read in both passes, s o r written by the first
ITERS_PER_CALL = 8


def med(fn, reps=7):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--preconditioner', choices=D.VARIABLE_DENSITY_PRECONDITIONERS, default='dst')
    ap.add_argument('--density-profile', choices=D.VARIABLE_DENSITY_PROFILES, default='abs')
    ap.add_argument('--ratio', type=float, default=10.0, help='max rho / min rho')
    ap.add_argument('--out', default=None, help='JSON file to write (default: profiles/varcoef_bench.json when every option has its default)')
    args = ap.parse_args()
    scaled = args.preconditioner == 'scaled'
    suffix = '_scaled' if scaled else ''
    model_bytes = dict(MODEL_BYTES, **(SCALED_BYTES if scaled else {}))
    density = K.varcoef_density_smooth if args.density_profile == 'smooth' else K.varcoef_density
    g = torch.Generator(device='cuda').manual_seed(0)
    gen = D.variable_density_dataset_generator(batch_size=1, density_range=(1.0, 10.0), seed=0)
    rows = []
    print('%-10s %5s %12s %12s %10s %10s %6s %12s %12s' % ('grid', 'batch', 'apply ms', 'iter ms', 'GB/s', 'GEMM TF/s', 'iters', 'solve ms/smp', 'dst ms/smp'))
    for n, N in ((256, 32), (512, 16), (1024, 8)):
        H = W = n
        per = (H - 2) * (W - 2)
        rng = np.random.default_rng(n)
        rhs = torch.randn(N, H, W, device='cuda', generator=g)
        rho = density(gen._smooth_field(2 * rng.uniform(size=(N, 6, 6)) - 1, (H, W), 1.0), 1.0, args.ratio)
        e = {k: torch.randn(N, H, device='cuda', generator=g) for k in ('left', 'right', 'bottom', 'top')}
        dx = torch.rand(N, device='cuda', generator=g) * 4.5e-2 + 5e-3
        p = torch.randn(N, H - 2, W - 2, device='cuda', dtype=torch.float64, generator=g)
        t_apply = med(lambda: K.varcoef_apply(rho, dx, p), 15)
        # one iteration: the state of a started solve, then calls that run ITERS_PER_CALL iterations each (a converged sample costs the same launches)
        Sh, lh = K.dst_matrices(H, rho.device)
        Sw, lw = K.dst_matrices(W, rho.device)
        lib = _lib.load()
        nbytes = int(lib.pcnn_varcoef_pcg_workspace_scaled(c_int(N), c_int(H), c_int(W)) if scaled else lib.pcnn_varcoef_pcg_workspace(c_int(N), c_int(H), c_int(W)))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
        scal = torch.empty((N, 8), dtype=torch.float64, device='cuda')
        flags = torch.empty((N,), dtype=torch.int32, device='cuda')
        h = handle()
        h.call('pcnn_varcoef_pcg_setup' + suffix, c_int(N), c_int(H), c_int(W), _p(rho), _p(rhs), _p(e['left']), _p(e['right']), _p(e['bottom']), _p(e['top']), _p(dx),
               None, c_double(1e-10), _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
        t_iter = med(lambda: h.call('pcnn_varcoef_pcg_iterate' + suffix, c_int(N), c_int(H), c_int(W), _p(rho), _p(dx), c_double(1e-10), c_int(0), c_int(ITERS_PER_CALL),
                                    _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))) / ITERS_PER_CALL
        info = {}

        def whole():
            info.update(D.variable_density_poisson_solve(rho, rhs, e, dx, tol=1e-10, return_info=True, preconditioner=args.preconditioner)[1])
        t_solve = med(whole, 3)
        t_dst = med(lambda: K.fd_poisson_dst(rhs, e['left'], e['right'], e['bottom'], e['top'], dx))
        model = sum(model_bytes.values()) * N * per
        flops = 4 * N * (H - 2) * (W - 2) * ((H - 2) + (W - 2))            # two products with S_h (2 nh^2 nw each), two with S_w (2 nh nw^2 each)
        row = {'grid': [H, W], 'batch': N, 'apply_ms': t_apply, 'apply_GBps': 20 * N * per / t_apply / 1e6, 'iteration_ms': t_iter,
               'iteration_model_bytes': model, 'iteration_model_GBps': model / t_iter / 1e6, 'iteration_gemm_TFLOPs': flops / t_iter / 1e9,
               'iterations': [int(v) for v in info['iterations']], 'converged': bool(info['converged'].all()), 'solve_ms_per_sample': t_solve / N,
               'fd_poisson_dst_ms_per_sample': t_dst / N}
        rows.append(row)
        print('%-10s %5d %12.4f %12.4f %10.0f %10.2f %6d %12.3f %12.3f' % ('%dx%d' % (H, W), N, t_apply, t_iter, row['iteration_model_GBps'],
                                                                           row['iteration_gemm_TFLOPs'], max(row['iterations']), row['solve_ms_per_sample'],
                                                                           row['fd_poisson_dst_ms_per_sample']))
    out = {'device': torch.cuda.get_device_name(0), 'source_hash': _lib.source_hash(), 'density_ratio': args.ratio, 'tol': 1e-10, 'iterations_per_call': ITERS_PER_CALL,
           'traffic_model_bytes_per_point_per_iteration': model_bytes, 'rows': rows}
    if (args.preconditioner, args.density_profile, args.ratio) != ('dst', 'abs', 10.0):
        out.update(preconditioner=args.preconditioner, density_profile=args.density_profile)
    path = args.out or (os.path.join(ROOT, 'profiles', 'varcoef_bench.json') if 'preconditioner' not in out else None)
    if path is None:
        return
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
