"""Times the variable-density solve with a reaction term (the *_reaction entry points of csrc/varcoef.hip) against the plain
*_bc_* solve of the same problem, at 512^2 with batch 16 and 1024^2 with batch 8 (mask 0): the operator launch (q = (A + C) p with its p.q; model 24 B
per point against 20) and one iteration of the loop (from calls of pcnn_varcoef_bc_pcg_iterate[_reaction] that run 8; model 176 B per point against
172), the two variants alternated, HIP-event medians after a warm-up call.  Then the iteration counts of whole solves at 512^2, tol = 1e-10, density
ratios 10 and 1000, for c = 0 (the plain solve), a small c and a large c: c = m s / (rho dx^2), s smooth in [0.5, 1.5], m = 0.1 and 1e3.
Writes the table to --out (default profiles/varcoef_reaction.txt).
--plain-only times the plain columns alone and calls nothing of the reaction family, so the same file measures a checkout - or, through PCNN_LIBRARY, a
build of the library - from before the term existed; name the file to write with --out."""
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


def alternated(fns, reps):
    """Median HIP-event time (ms) of each callable, one warm-up call each, the callables taking turns."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e))
    return [float(np.median(t)) for t in ts]


def fields(gen, n, N, ratio, g, plain_only=False):
    H = W = n
    rng = np.random.default_rng(n)
    rhs = torch.randn(N, H, W, device='cuda', generator=g)
    rho = K.varcoef_density(gen._smooth_field(2 * rng.uniform(size=(N, 6, 6)) - 1, (H, W), 1.0), 1.0, ratio)
    shape = gen._smooth_field(2 * rng.uniform(size=(N, 5, 5)) - 1, (H, W), 1.0)            # (drawn in either mode: the same streams)
    e = {k: torch.randn(N, H, device='cuda', generator=g) for k in EDGES}
    dx = torch.rand(N, device='cuda', generator=g) * 4.5e-2 + 5e-3
    return rhs, rho, None if plain_only else K.varcoef_reaction_field(shape, 0.5, 1.5) / (rho * (dx * dx).view(N, 1, 1)), e, dx


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_reaction.txt'))
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--plain-only', action='store_true', help='the plain *_bc_* columns alone: nothing of the reaction family is called')
    args = ap.parse_args()
    po = args.plain_only
    g = torch.Generator(device='cuda').manual_seed(0)
    gen = D.variable_density_dataset_generator(batch_size=1, density_range=(1.0, 10.0), seed=0)
    lib, h = _lib.load(), handle()
    lines = ['%s, mask 0, tol 1e-10, %d iterations per call, %d alternated timings per figure, %s'
             % (torch.cuda.get_device_name(0), ITERS_PER_CALL, args.repeats,
                'library %s, plain columns only' % os.path.basename(_lib.LIB_PATH) if po else 'source %s' % _lib.source_hash()), '',
             '%-10s %5s %14s %14s %7s %14s %14s %7s' % ('grid', 'batch', 'apply ms', 'apply+c ms', 'ratio', 'iter ms', 'iter+c ms', 'ratio')]
    for n, N in ((512, 16), (1024, 8)):
        H = W = n
        rhs, rho, unit, e, dx = fields(gen, n, N, 10.0, g, po)
        c = None if po else (10.0 * unit).contiguous()
        p = torch.randn(N, H - 2, W - 2, device='cuda', dtype=torch.float64, generator=g)
        none = (False,) * 4
        t_apply = alternated([lambda: K.varcoef_apply(rho, dx, p, neumann=none)] + ([] if po else [lambda: K.varcoef_apply(rho, dx, p, neumann=none, reaction=c)]),
                             2 * args.repeats)
        Vih, Vh, lh, ViwT, VwT, lw = K._varcoef_bases(H, W, none, rho.device)
        state = {}
        for name in ('',) if po else ('', '_reaction'):
            nbytes = int(lib.pcnn_varcoef_bc_pcg_workspace_reaction(c_int(N), c_int(H), c_int(W), c_int(0)) if name else
                         lib.pcnn_varcoef_bc_pcg_workspace(c_int(N), c_int(H), c_int(W), c_int(0)))
            state[name] = (torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda'), nbytes, torch.empty((N * 12,), dtype=torch.float64, device='cuda'),
                           torch.empty((N,), dtype=torch.int32, device='cuda'))
        ws, nb, scal, flags = state['']
        h.call('pcnn_varcoef_bc_pcg_setup', c_int(N), c_int(H), c_int(W), c_int(0), _p(rho), _p(rhs), _p(e['left']), _p(e['right']), _p(e['bottom']), _p(e['top']),
               _p(dx), None, c_double(1e-10), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nb), _p(scal), _p(flags))
        if not po:
            ws, nb, scal, flags = state['_reaction']
            h.call('pcnn_varcoef_bc_pcg_setup_reaction', c_int(N), c_int(H), c_int(W), c_int(0), _p(rho), _p(rhs), _p(e['left']), _p(e['right']), _p(e['bottom']),
                   _p(e['top']), _p(dx), None, c_double(1e-10), _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nb), _p(scal), _p(flags), _p(c))

        def plain():
            ws, nb, scal, flags = state['']
            h.call('pcnn_varcoef_bc_pcg_iterate', c_int(N), c_int(H), c_int(W), c_int(0), _p(rho), _p(dx), c_double(1e-10), c_int(0), c_int(ITERS_PER_CALL), _p(Vih),
                   _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nb), _p(scal), _p(flags))

        def with_c():
            ws, nb, scal, flags = state['_reaction']
            h.call('pcnn_varcoef_bc_pcg_iterate_reaction', c_int(N), c_int(H), c_int(W), c_int(0), _p(rho), _p(dx), c_double(1e-10), c_int(0), c_int(ITERS_PER_CALL),
                   _p(Vih), _p(Vh), _p(lh), _p(ViwT), _p(VwT), _p(lw), _p(ws), c_size_t(nb), _p(scal), _p(flags), _p(c))
        t_iter = [t / ITERS_PER_CALL for t in alternated([plain] if po else [plain, with_c], args.repeats)]
        if po:
            t_apply, t_iter = t_apply * 2, t_iter * 2                          # (the +c columns repeat the plain ones: ratio 1)
        lines.append('%-10s %5d %14.4f %14.4f %7.3f %14.4f %14.4f %7.3f' % ('%dx%d' % (H, W), N, t_apply[0], t_apply[1], t_apply[1] / t_apply[0], t_iter[0], t_iter[1],
                                                                           t_iter[1] / t_iter[0]))
        print(lines[-1], flush=True)
    lines += ['', 'iterations to tol 1e-10 at 512x512, batch 4 (the device looks every %d): c = m s / (rho dx^2), s in [0.5, 1.5]' % ITERS_PER_CALL,
              '%-8s %-22s %-22s %-22s' % ('ratio', 'c = 0 (plain solve)', 'm = 0.1', 'm = 1e3')]
    for ratio in (10.0, 1000.0):
        rhs, rho, unit, e, dx = fields(gen, 512, 4, ratio, g, po)
        counts = []
        for m in (None,) if po else (None, 0.1, 1e3):
            extra = {} if m is None else {'reaction': (m * unit).contiguous()}
            info = D.variable_density_poisson_solve(rho, rhs, e, dx, tol=1e-10, return_info=True, **extra)[1]
            counts.append('%r%s' % (info['iterations'].tolist(), '' if info['converged'].all() else ' (not converged)'))
        lines.append('%-8g %-22s %-22s %-22s' % (ratio, *(counts + ['-', '-'])[:3]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
