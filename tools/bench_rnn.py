"""Dirichlet_BC_RNN (configs.dbcnn_rnn() = experiments/dbcnn_rnn.json: batch 50, six layers of 100 units) on the persistent recurrence kernels, as an
LSTM and as a GRU, at T = 192 and T = 384 (the two ends of the shipped shape range; the output is T x T):

  - HIP-event time of every recurrence launch, forward and backward (ops.KernelTimer around each launch, a run of its own), the resulting
    microseconds per time step, and the time-parallel launches (projection, dX, dW / dU / db) of the same steps;
  - one whole train step and one inference call, host clock around work that ends in a device synchronise;
  - the shipped workload: model.fit on the numerical generator, a new shape in [192, 384]^2 every batch, as train.main runs it;
  - for scale, torch.nn.LSTM / torch.nn.GRU (MIOpen through torch-ROCm; this tool only, the library never imports them) on the same shapes, six
    stacked layers, forward and forward + backward.

No threshold is applied to any of these.

    python tools/bench_rnn.py [--steps 5] [--warmup 2] [--shipped-steps 8] [--out profiles/rnn_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {'median_ms': t[len(t) // 2], 'min_ms': t[0], 'max_ms': t[-1], 'steps': steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--shipped-steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from poisson_cnn_amd import configs, ops
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.rnn import Dirichlet_BC_RNN
    from poisson_cnn_amd.train import choose_optimizer
    if not torch.cuda.is_available():
        raise SystemExit('bench_rnn.py measures on the GPU; none found')
    cfg = configs.dbcnn_rnn()
    N = cfg['dataset']['batch_size']
    units = cfg['model']['units']
    res = {'device': torch.cuda.get_device_name(0), 'batch': N, 'units': units, 'cases': []}
    for cell in ('lstm', 'gru'):
        model = Dirichlet_BC_RNN(**dict(cfg['model'], RNN_type=cell))
        model.compile(loss=loss_wrapper(global_batch_size=N, **cfg['training']['loss_parameters']),
                      optimizer=choose_optimizer(cfg['training']['optimizer'])(**cfg['training']['optimizer_parameters']), max_input_shape=(N, 384, 384))
        for T in (192, 384):
            rng = np.random.default_rng(T)
            bc = torch.from_numpy((np.cumsum(rng.standard_normal((N, 1, T)), 2) * 0.1).astype(np.float32)).cuda()
            dx = torch.full((N, 1), 0.02, device='cuda')
            y = torch.from_numpy(rng.uniform(-0.5, 0.5, (N, 1, T, T)).astype(np.float32)).cuda()
            data = ((bc, dx), y)
            case = {'cell': cell, 'T': T, 'X': T}
            case['train_step'] = timed(lambda: model.train_step(data), args.steps, args.warmup)
            case['inference'] = timed(lambda: model([bc, dx, T]), args.steps, args.warmup)
            # per-launch HIP events, in steps of their own
            timer = ops.KernelTimer()
            ops.set_kernel_timer(timer)
            for _ in range(args.steps):
                model.train_step(data)
            ops.set_kernel_timer(None)
            kinds = {}
            for kind in ('rnn_fwd', 'rnn_bwd', 'wide_fwd', 'wide_dgrad', 'wide_wgrad', 'resize_fwd'):
                _, sec, n = timer.totals(kind)
                if n:
                    kinds[kind] = {'launches_per_step': n / args.steps, 'ms_per_step': sec * 1e3 / args.steps, 'us_per_launch': sec * 1e6 / n}
            for kind in ('rnn_fwd', 'rnn_bwd'):
                kinds[kind]['us_per_time_step'] = kinds[kind]['us_per_launch'] / T
            case['kernels'] = kinds
            # MIOpen through torch.nn, six stacked layers of the same widths
            mods, cin = [], 1
            for u in units:
                mods.append((torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(cin, u, batch_first=True).cuda())
                cin = u
            xt = bc.permute(0, 2, 1).contiguous()
            gy = torch.randn(N, T, units[-1], device='cuda')

            def vendor(backward):
                o = xt
                if backward:
                    for m in mods:
                        m.zero_grad(set_to_none=True)
                for m in mods:
                    o = m(o)[0]
                if backward:
                    (o * gy).sum().backward()
            with torch.no_grad():
                case['torch_nn_forward'] = timed(lambda: vendor(False), args.steps, args.warmup)
            case['torch_nn_forward_backward'] = timed(lambda: vendor(True), args.steps, args.warmup)
            ours_f = kinds['rnn_fwd']['ms_per_step'] + kinds['wide_fwd']['ms_per_step']
            ours_fb = ours_f + kinds['rnn_bwd']['ms_per_step'] + kinds['wide_dgrad']['ms_per_step'] + kinds['wide_wgrad']['ms_per_step']
            case['rnn_stack_kernel_ms'] = {'forward': ours_f, 'forward_backward': ours_fb}
            res['cases'].append(case)
            print('%-4s T=%d: train step %.2f ms, inference %.2f ms | recurrence fwd %.1f us/launch (%.3f us/step), bwd %.1f us/launch (%.3f us/step) | '
                  'stack kernels fwd %.2f ms, fwd+bwd %.2f ms | torch.nn fwd %.2f ms, fwd+bwd %.2f ms'
                  % (cell, T, case['train_step']['median_ms'], case['inference']['median_ms'], kinds['rnn_fwd']['us_per_launch'],
                     kinds['rnn_fwd']['us_per_time_step'], kinds['rnn_bwd']['us_per_launch'], kinds['rnn_bwd']['us_per_time_step'], ours_f, ours_fb,
                     case['torch_nn_forward']['median_ms'], case['torch_nn_forward_backward']['median_ms']), flush=True)
        del model
    # the shipped workload: shape changes every batch, the generator on the device, fit() as train.main runs it
    if args.shipped_steps > 0:
        from poisson_cnn_amd.dataset import numerical_dataset_generator
        d = dict(cfg['dataset'], batches_per_epoch=args.shipped_steps)
        ds = numerical_dataset_generator(randomize_boundary_smoothness=True, exclude_zero_boundaries=True, nonzero_boundaries=['left'], rhses='zero',
                                         return_boundaries=True, return_dx=True, return_rhs=False, **d)
        model = Dirichlet_BC_RNN(**cfg['model'])
        model.compile(loss=loss_wrapper(global_batch_size=N, **cfg['training']['loss_parameters']),
                      optimizer=choose_optimizer(cfg['training']['optimizer'])(**cfg['training']['optimizer_parameters']), max_input_shape=(N, 384, 384))
        model.fit(ds, epochs=1, verbose=0)                                          # warm-up epoch: generator set-up, per-shape tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit(ds, epochs=1, verbose=0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res['shipped_workload'] = {'steps': args.shipped_steps, 'ms_per_step': dt * 1e3 / args.shipped_steps, 'grids_per_s': N * args.shipped_steps / dt}
        print('shipped workload (new shape every batch): %.1f ms/step, %.0f grids/s' % (dt * 1e3 / args.shipped_steps, N * args.shipped_steps / dt), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({'rnn_bench': 'done', 'cases': len(res['cases'])}))


if __name__ == '__main__':
    main()
