"""What starting the variable-density conjugate-gradient solve from a model's prediction costs and saves: a record, not a
gate - no threshold is applied and no saving is promised.  CG started at x0 gains about log(||e0 cold|| / ||e0 warm||) iterations, so an untrained
prediction may gain nothing, or cost iterations.

Fixed seed; variable_density_dataset_generator at density ratio 10 and 100; one small (2 x 64 x 72) and one 512^2 (4 x 512 x 512) batch.  Per case:
  cold                       variable_density_poisson_solve started at 0
  warm, untrained            ... started at the prediction of a freshly initialised Homogeneous_Poisson_NN_Legacy(density_input=True) (tiny config)
  warm, after a short fit    ... of the same model after --fit_steps Adam steps on the generator at this shape and ratio
with the iterations per sample (a multiple of check_every = 8, 0 when the start already meets tol), the prediction's rel-L2 error and relative
residual (ops.varcoef_error_stats), and the time of the solver call alone - the forward pass is timed separately - as the median of --repeats
HIP-event timings, cold and warm alternating, with the spread (max - min) / median.  The solve reads its convergence flags on the host every
check_every iterations; those round trips are inside the timing, as they are for a user.

Then pcnn_varcoef_error_stats alone: --calls back-to-back calls between two events, median of --repeats, against its traffic model of 16 B per point
(pred, target, rho, rhs once each; the neighbour rows come from cache) and 0.79 x the HBM peak (the copy figure of DESIGN.md section 4).  The file
says for every shape whether its four tensors fit the 256 MB Infinity Cache: where they do, the rate is not an HBM rate.

    python tools/bench_varcoef_warmstart.py [--fit_steps 40] [--repeats 5] [--calls 20] [--out profiles/varcoef_warmstart.txt (the default)]
"""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X
COPY_FRACTION = 0.79
INFINITY_CACHE_MB = 256.0
SEED = 18


def median_spread(t):
    t = sorted(t)
    med = t[len(t) // 2]
    return med, (t[-1] - t[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fit_steps', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'varcoef_warmstart.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from poisson_cnn_amd import configs, dataset as D, ops
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    from poisson_cnn_amd.train import Adam
    if not torch.cuda.is_available():
        raise SystemExit('bench_varcoef_warmstart.py measures on the GPU; none found')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    say('tools/bench_varcoef_warmstart.py on %s: seed %d, fit_steps %d, repeats %d, tol 1e-10, check_every 8' % (torch.cuda.get_device_name(0), SEED,
                                                                                                              args.fit_steps, args.repeats))
    say('A record, not a gate: warm-start savings are measured here, not promised.')
    full = configs.hpnn_tiny()
    lossp = dict(full['training']['loss_parameters'])
    lossp.update(physics_informed_loss_weight=1e-9, mse_loss_weight=0.2, physics_informed_loss_config={'stencil_sizes': [3, 3], 'orders': 2, 'normalize': False})
    for (N, H, W) in ((2, 64, 72), (4, 512, 512)):
        for ratio in (10.0, 100.0):
            gen = D.variable_density_dataset_generator(batch_size=N, batches_per_epoch=args.fit_steps, output_shape=(H, W), density_range=(1.0, ratio), seed=SEED)
            (stack, dx), soln = gen[0]                                      # the batch every start is measured on; fit sees the batches after it
            rhs, rho = stack[:, 0].contiguous(), stack[:, 1].contiguous()
            zero = {k: torch.zeros((N, W if k in ('left', 'right') else H), device=stack.device) for k in ('left', 'right', 'bottom', 'top')}
            model = Homogeneous_Poisson_NN_Legacy(**dict(full['model'], density_input=True, postsmoother_iterations=2, seed=SEED))
            say()
            say('%d x %d x %d, density ratio %g (four fields: %.1f MB)' % (N, H, W, ratio, 4 * N * H * W * 4 / 1e6))
            cold_its = None
            for stage in ('untrained', 'after %d Adam steps' % args.fit_steps):
                if stage != 'untrained':
                    model.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **lossp), optimizer=Adam(learning_rate=1e-3))
                    hist = model.fit(gen, epochs=1, verbose=0)
                    say('  fit: last-batch loss %.4g' % float(hist['loss'][-1]))
                pred = model([stack, dx])
                t_fwd = median_spread([timed(lambda: model([stack, dx]))[0] for _ in range(args.repeats)])
                st = ops.varcoef_error_stats(pred, rho, soln, rhs, dx.reshape(-1)).cpu().numpy().astype(np.float64)
                rel_l2, rel_res = np.sqrt(st[:, 1] / st[:, 3]), np.sqrt(st[:, 5] / st[:, 7])
                solve = lambda x0: D.variable_density_poisson_solve(rho, rhs, zero, dx, initial_guesses=x0, return_info=True, check_start=True)
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore', RuntimeWarning)             # a sample that runs out of iterations shows in the table
                    solve(None), solve(pred)                                    # warm-up of both
                    times, infos = {'cold': [], 'warm': []}, {}
                    for _ in range(args.repeats):
                        for name, x0 in (('cold', None), ('warm', pred)):
                            t, (_, infos[name]) = timed(lambda: solve(x0))
                            times[name].append(t)
                    _, whole = model.solve([stack, dx], return_info=True)
                if cold_its is None:
                    cold_its = infos['cold']['iterations']
                    m, s = median_spread(times['cold'])
                    say('  cold:                      iterations %-22r %8.2f ms (spread %4.1f%%)  converged %r' % (cold_its.tolist(), m, 100 * s,
                                                                                                                 infos['cold']['converged'].tolist()))
                assert np.array_equal(whole['iterations'], infos['warm']['iterations'])
                m, s = median_spread(times['warm'])
                say('  warm, %-20s iterations %-22r %8.2f ms (spread %4.1f%%)  converged %r' % (stage + ':', infos['warm']['iterations'].tolist(), m, 100 * s,
                                                                                              infos['warm']['converged'].tolist()))
                say('        prediction rel-L2 %s, relative residual %s; forward %.2f ms (spread %.1f%%)' % (
                    np.array2string(rel_l2, precision=3), np.array2string(rel_res, precision=3), t_fwd[0], 100 * t_fwd[1]))
    say()
    say('pcnn_varcoef_error_stats, %d calls per timing, traffic model 16 B per point' % args.calls)
    for (N, H, W) in ((2, 64, 72), (4, 512, 512), (8, 1024, 1024), (32, 1024, 1024)):
        g = torch.Generator(device='cuda').manual_seed(SEED)
        pred, target, rhs = (torch.randn(N, H, W, device='cuda', generator=g) for _ in range(3))
        rho = torch.rand(N, H, W, device='cuda', generator=g) * 9 + 1
        dx = torch.rand(N, device='cuda', generator=g) * 0.045 + 0.005
        for _ in range(3):
            ops.varcoef_error_stats(pred, rho, target, rhs, dx)
        torch.cuda.synchronize()
        med, spread = median_spread([timed(lambda: [ops.varcoef_error_stats(pred, rho, target, rhs, dx) for _ in range(args.calls)])[0] / args.calls
                                     for _ in range(args.repeats + 2)])
        mb = 16.0 * N * H * W / 1e6
        rate = mb / 1e3 / (med * 1e-3)
        say('  %2d x %4d x %4d: %8.4f ms (spread %4.1f%%)  %7.1f MB = %6.0f GB/s = %.2f of the copy rate; the four tensors %s the %d MB Infinity Cache' % (
            N, H, W, med, 100 * spread, mb, rate, rate / (COPY_FRACTION * HBM_PEAK_GBPS), 'fit' if mb <= INFINITY_CACHE_MB else 'do NOT fit', INFINITY_CACHE_MB))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
