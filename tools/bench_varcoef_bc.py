"""Times the variable-density Poisson solve with per-edge Dirichlet / Neumann boundaries (the *_bc_* entry points of csrc/varcoef.hip, DESIGN.md
section 19) at 8 x 512^2: for the masks 0, 5 (left and bottom Neumann) and 15 (all Neumann) and the density ratios 10 and 100, one iteration of the
preconditioned conjugate-gradient loop (from a call of pcnn_varcoef_bc_pcg_iterate that runs 8; HIP-event median after a warm-up call) and the
iterations a whole solve needs to tol = 1e-10 - and the same two figures for mask 0 through the all-Dirichlet entry points, the path every solve took
before.  --old-only times that path alone and uses nothing newer than it, so the same file measures an older checkout on the same device.
--preconditioner scaled takes the *_scaled entry points, --density-profile smooth the generator's smooth profile.
A record, no threshold.  Prints a table; --out writes it as text (profiles/varcoef_bc.txt is such a record)."""
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
N, H, W = 8, 512, 512
EDGES = ('left', 'right', 'bottom', 'top')


def med(fn, reps=9):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def iteration_ms(rho, rhs, e, dx, mask, scaled=False):
    """ms per iteration of a started solve; mask None: the all-Dirichlet entry points."""
    lib, h = _lib.load(), handle()
    scal = torch.empty((N, 8), dtype=torch.float64, device='cuda')
    flags = torch.empty((N,), dtype=torch.int32, device='cuda')
    shape = (c_int(N), c_int(H), c_int(W))
    edges = tuple(_p(e[k]) for k in EDGES)
    if mask is None:
        Sh, lh = K.dst_matrices(H, rho.device)
        Sw, lw = K.dst_matrices(W, rho.device)
        bases = (_p(Sh), _p(lh), _p(Sw), _p(lw))
        nbytes = int(lib.pcnn_varcoef_pcg_workspace_scaled(*shape) if scaled else lib.pcnn_varcoef_pcg_workspace(*shape))
        name = 'pcnn_varcoef_pcg_'
    else:
        shape += (c_int(mask),)
        bases = tuple(_p(t) for t in K._varcoef_bases(H, W, tuple(bool(mask >> k & 1) for k in range(4)), rho.device))
        nbytes = int(lib.pcnn_varcoef_bc_pcg_workspace_scaled(*shape) if scaled else lib.pcnn_varcoef_bc_pcg_workspace(*shape))
        name = 'pcnn_varcoef_bc_pcg_'
    suffix = '_scaled' if scaled else ''
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
    h.call(name + 'setup' + suffix, *shape, _p(rho), _p(rhs), *edges, _p(dx), None, c_double(1e-10), *bases, _p(ws), c_size_t(nbytes), _p(scal), _p(flags))
    t = med(lambda: h.call(name + 'iterate' + suffix, *shape, _p(rho), _p(dx), c_double(1e-10), c_int(0), c_int(ITERS_PER_CALL), *bases, _p(ws), c_size_t(nbytes), _p(scal),
                           _p(flags)))
    return tuple(v / ITERS_PER_CALL for v in t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--old-only', action='store_true', help='only mask 0 through the all-Dirichlet entry points')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--preconditioner', choices=('dst', 'scaled'), default='dst')
    ap.add_argument('--density-profile', choices=('abs', 'smooth'), default='abs')
    args = ap.parse_args()
    scaled = args.preconditioner == 'scaled'
    pre = {'preconditioner': 'scaled'} if scaled else {}              # (the defaults spell every call as an older checkout takes it)
    density = K.varcoef_density_smooth if args.density_profile == 'smooth' else K.varcoef_density
    g = torch.Generator(device='cuda').manual_seed(0)
    gen = D.variable_density_dataset_generator(batch_size=1, density_range=(1.0, 10.0), seed=0)
    rhs = torch.randn(N, H, W, device='cuda', generator=g)
    e = {k: torch.randn(N, H, device='cuda', generator=g) for k in EDGES}
    dx = torch.rand(N, device='cuda', generator=g) * 4.5e-2 + 5e-3
    lines = ['%s, %d x %d x %d, tol 1e-10, %d iterations per call, source %s' % (torch.cuda.get_device_name(0), N, H, W, ITERS_PER_CALL, _lib.source_hash())
             + ('' if (args.preconditioner, args.density_profile) == ('dst', 'abs') else ', preconditioner %s, density profile %s' % (args.preconditioner, args.density_profile)),
             '%-34s %9s %26s %12s %14s' % ('path', 'rho ratio', 'ms / iteration (min..max)', 'iterations', 'solve ms / smp')]
    for ratio in (10.0, 100.0):
        rng = np.random.default_rng(512)
        rho = density(gen._smooth_field(2 * rng.uniform(size=(N, 6, 6)) - 1, (H, W), 1.0), 1.0, ratio)
        cases = [('mask 0, all-Dirichlet entry points', None)] + ([] if args.old_only else [('mask %d, *_bc_* entry points' % m, m) for m in (0, 5, 15)])
        for label, mask in cases:
            t, lo, hi = iteration_ms(rho, rhs, e, dx, mask, scaled)
            info = {}
            if mask is None:
                whole = lambda: info.update(D.variable_density_poisson_solve(rho, rhs, e, dx, tol=1e-10, return_info=True, **pre)[1])
            else:
                whole = lambda: info.update(K.varcoef_pcg_solve(rho, rhs, e['left'], e['right'], e['bottom'], e['top'], dx, tol=1e-10,
                                                                neumann=tuple(bool(mask >> k & 1) for k in range(4)), **({'scaled': True} if scaled else {}))[1])
            t_solve = med(whole, 3)[0]
            lines.append('%-34s %9g %12.4f (%.4f..%.4f) %12s %14.3f' % (label, ratio, t, lo, hi, '%d..%d' % (info['iterations'].min(), info['iterations'].max()),
                                                                       t_solve / N) + ('' if info['converged'].all() else '  NOT CONVERGED'))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
