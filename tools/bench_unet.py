"""UNet baseline (configs.unet() = experiments/UNet.json) on the wide-channel kernels: train step and inference at the worst case 50 x 384^2, and
grids/s on the shipped workload (batch 50, a new grid shape in [192, 384]^2 every batch, analytic generator on the device, model.fit as train.main
runs it).  Per-kind kernel time comes from HIP events around every launch (ops.KernelTimer) in a run of its own, with the FLOPs of each launch
computed from its shapes (ops._launch); the fraction is against the 157.3 TFLOP/s fp32 matrix peak.  For the per-kernel table run the same tool
under `rocprofv3 --kernel-trace --stats -- python tools/bench_unet.py --mode trace` (no timing is taken from that run).

    python tools/bench_unet.py [--mode all|trace] [--steps 3] [--shipped-steps 12] [--out profiles/unet_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX = 157.3e12


def unet_flops(model, N, H, W):
    """Forward multiply-add FLOPs of one batch, counted from layer shapes (2 per MAC)."""
    from poisson_cnn_amd import ops
    sizes = [(H, W)]
    for _ in range(model.depth - 1):
        sizes.append((ops.pool_out(sizes[-1][0], model.pool), ops.pool_out(sizes[-1][1], model.pool)))
    f = 0.0
    for i, blk in enumerate(model.down + [model.bottom]):
        h, w = sizes[i]
        for (_, _, ci, co, k) in blk:
            f += 2.0 * N * h * w * k * k * ci * co
    for j, ((_, _, ci, co), blk) in enumerate(model.up):
        i = model.depth - 2 - j
        h, w = sizes[i]
        f += 2.0 * N * ops.pool_out(h, model.pool) * ops.pool_out(w, model.pool) * model.pool ** 2 * ci * co
        for (_, _, ci2, co2, k) in blk:
            f += 2.0 * N * h * w * k * k * ci2 * co2
    _, _, ci, co, k = model.head
    return f + 2.0 * N * H * W * ci * co


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', default='all', choices=['all', 'trace'])
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shipped-steps', type=int, default=12)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from poisson_cnn_amd import configs, ops
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator
    from poisson_cnn_amd.losses import loss_wrapper
    from poisson_cnn_amd.train import choose_optimizer
    from poisson_cnn_amd.unet import UNet
    cfg = configs.unet()
    N, H, W = 50, 384, 384
    model = UNet(**cfg['model'])
    model.compile(loss=loss_wrapper(global_batch_size=N, **cfg['training']['loss_parameters']),
                  optimizer=choose_optimizer('adam')(**cfg['training']['optimizer_parameters']), max_input_shape=(N, H, W))
    g = torch.Generator(device='cpu').manual_seed(0)
    rhs = (torch.rand(N, 1, H, W, generator=g) * 2 - 1).cuda()
    dx = torch.full((N, 1), 0.01, device='cuda')
    y = (torch.rand(N, 1, H, W, generator=g) * 0.1).cuda()
    fwd = unet_flops(model, N, H, W)
    res = {'workload': 'unet UNet.json 50x384^2', 'fwd_tflop': fwd / 1e12, 'step_tflop': 3 * fwd / 1e12}
    if args.mode == 'trace':
        for _ in range(2):
            model.train_step(((rhs, dx), y))
        with torch.no_grad():
            model(rhs)
        torch.cuda.synchronize()
        print(json.dumps(res))
        return
    for _ in range(args.warmup):
        model.train_step(((rhs, dx), y))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        logs = model.train_step(((rhs, dx), y))
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / args.steps
    res.update(train_step_ms=step * 1e3, train_step_tflops=3 * fwd / step / 1e12, loss=float(logs['loss']))
    model(rhs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model(rhs)
    torch.cuda.synchronize()
    inf = (time.perf_counter() - t0) / args.steps
    res.update(inference_ms=inf * 1e3, inference_tflops=fwd / inf / 1e12)
    # per-kind kernel time of one train step (its own run: the events serialise nothing but add launch gaps)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    model.train_step(((rhs, dx), y))
    ops.set_kernel_timer(None)
    kinds = {}
    for kind in sorted({r[0] for r in timer.records}):
        fl, sec, n = timer.totals(kind)
        kinds[kind] = {'launches': n, 'ms': sec * 1e3, 'tflops': fl / max(sec, 1e-12) / 1e12, 'frac_fp32_matrix_peak': fl / max(sec, 1e-12) / PEAK_FP32_MATRIX}
    # the 3x3 layers with Cin, Cout >= 64 alone (the bar of the design notes)
    big = lambda k, f, b: k in ('wide_fwd', 'wide_dgrad', 'wide_wgrad')     # noqa: E731
    fl, _, sec, n = timer.select(big)
    res['kinds'] = kinds
    res['wide_conv_all'] = {'ms': sec * 1e3, 'frac_fp32_matrix_peak': fl / sec / PEAK_FP32_MATRIX}
    # shipped workload: fit() on the analytic generator, a new shape every batch
    dcfg = dict(cfg['dataset'], batches_per_epoch=args.shipped_steps)
    ds = reverse_poisson_dataset_generator(**dcfg)
    ends = []

    class Rec:
        def set_model(self, m):
            pass

        def on_batch_end(self, b, logs):
            ends.append(time.perf_counter())

        def on_epoch_end(self, e, logs):
            pass
    t0 = time.perf_counter()
    model.fit(ds, epochs=1, callbacks=[Rec()], verbose=0)
    torch.cuda.synchronize()
    steady = np.diff(ends[1:]) if len(ends) > 2 else np.array([time.perf_counter() - t0])
    res.update(shipped_step_ms=float(np.mean(steady)) * 1e3, shipped_grids_per_s=N / float(np.mean(steady)), shipped_steps=len(ends))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
