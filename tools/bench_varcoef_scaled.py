"""The diagonally scaled preconditioner of the variable-density solve (preconditioner='scaled') against the plain one
('dst') on the same device, in one process:
  1. ms per iteration at 32 x 256^2, 16 x 512^2 and 8 x 1024^2 (the shapes and inputs of tools/bench_varcoef.py, whose record
     profiles/varcoef_bench.json is the yardstick for 'dst'): calls of pcnn_varcoef_pcg_iterate[_scaled] that run 8 iterations, HIP-event medians
     of 9 calls after a warm-up call, the two entry points measured alternately (A B A B, two rounds) so that clock drift shows as the spread
     between rounds and not as a difference between them;
  2. iterations and ms of a whole solve to tol = 1e-10 at 8 x 512^2 for the density ratios 10, 100 and 1000, the generator's 'abs' (kinked) and
     'smooth' profiles and both preconditioners - the unfavourable rows included.
A record, no threshold.  Prints a table; --out writes it as text (profiles/varcoef_scaled.txt is such a record)."""
import argparse
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

ITERS_PER_CALL = 8
EDGES = ('left', 'right', 'bottom', 'top')


def med(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def started_solve(rho, rhs, e, dx, scaled):
    """-> a closure that runs ITERS_PER_CALL iterations of a solve set up here (a converged sample costs the same launches)."""
    N, H, W = rho.shape
    lib, h = _lib.load(), handle()
    Sh, lh = K.dst_matrices(H, rho.device)
    Sw, lw = K.dst_matrices(W, rho.device)
    nbytes = int(lib.pcnn_varcoef_pcg_workspace_scaled(c_int(N), c_int(H), c_int(W)) if scaled else lib.pcnn_varcoef_pcg_workspace(c_int(N), c_int(H), c_int(W)))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
    scal = torch.empty((N, 8), dtype=torch.float64, device='cuda')
    flags = torch.empty((N,), dtype=torch.int32, device='cuda')
    suffix = '_scaled' if scaled else ''
    h.call('pcnn_varcoef_pcg_setup' + suffix, c_int(N), c_int(H), c_int(W), _p(rho), _p(rhs), *[_p(e[k]) for k in EDGES], _p(dx), None, c_double(1e-10), _p(Sh),
           _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
    return lambda: h.call('pcnn_varcoef_pcg_iterate' + suffix, c_int(N), c_int(H), c_int(W), _p(rho), _p(dx), c_double(1e-10), c_int(0), c_int(ITERS_PER_CALL),
                          _p(Sh), _p(lh), _p(Sw), _p(lw), _p(ws), c_size_t(nbytes), _p(scal), _p(flags))


def inputs(n, N, g):
    rhs = torch.randn(N, n, n, device='cuda', generator=g)
    e = {k: torch.randn(N, n, device='cuda', generator=g) for k in EDGES}
    dx = torch.rand(N, device='cuda', generator=g) * 4.5e-2 + 5e-3
    return rhs, e, dx


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()
    gen = D.variable_density_dataset_generator(batch_size=1, density_range=(1.0, 10.0), seed=0)
    field = lambda n, N: gen._smooth_field(2 * np.random.default_rng(n).uniform(size=(N, 6, 6)) - 1, (n, n), 1.0)
    lines = []

    def say(*rows):
        for row in rows:
            lines.append(row)
            print(row, flush=True)
    say('%s, tol 1e-10, %d iterations per call, source %s' % (torch.cuda.get_device_name(0), ITERS_PER_CALL, _lib.source_hash()), '',
        '1. ms per iteration, median (min..max) of 9 calls, rounds in the order dst, scaled, dst, scaled; abs profile, ratio 10',
        '%-12s %5s %28s %28s %8s' % ('grid', 'batch', 'dst', 'scaled', 'ratio'))
    g = torch.Generator(device='cuda').manual_seed(0)
    for n, N in ((256, 32), (512, 16), (1024, 8)):
        rhs, e, dx = inputs(n, N, g)
        rho = K.varcoef_density(field(n, N), 1.0, 10.0)
        run = {False: started_solve(rho, rhs, e, dx, False), True: started_solve(rho, rhs, e, dx, True)}
        for rnd in range(2):
            t = {sc: tuple(v / ITERS_PER_CALL for v in med(run[sc], 9)) for sc in (False, True)}
            say('%-12s %5d %12.4f (%.4f..%.4f) %12.4f (%.4f..%.4f) %8.3f' % ('%dx%d' % (n, n), N, *t[False], *t[True], t[True][0] / t[False][0]))
        del run
    say('', '2. whole solve, 8 x 512 x 512: iterations (min..max over the batch; looks of 8) and ms per sample (median of 3)',
        '%-8s %6s %16s %16s %14s %14s' % ('profile', 'ratio', 'dst iterations', 'scaled iters', 'dst ms/smp', 'scaled ms/smp'))
    n, N = 512, 8
    rhs, e, dx = inputs(n, N, g)
    for profile in ('smooth', 'abs'):
        for ratio in (10.0, 100.0, 1000.0):
            rho = (K.varcoef_density_smooth if profile == 'smooth' else K.varcoef_density)(field(n, N), 1.0, ratio)
            cell = {}
            for pre in ('dst', 'scaled'):
                info = {}
                t = med(lambda: info.update(D.variable_density_poisson_solve(rho, rhs, e, dx, tol=1e-10, max_iterations=2000, return_info=True, preconditioner=pre)[1]), 3)[0]
                cell[pre] = ('%d..%d%s' % (info['iterations'].min(), info['iterations'].max(), '' if info['converged'].all() else ' (!)'), t / N)
            say('%-8s %6g %16s %16s %14.3f %14.3f' % (profile, ratio, cell['dst'][0], cell['scaled'][0], cell['dst'][1], cell['scaled'][1]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
