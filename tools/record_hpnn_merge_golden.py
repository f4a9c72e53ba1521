"""Records what Homogeneous_Poisson_NN_Legacy's forward and backward return on the tiny model, and what the boundary-ring operators return, for
tests/test_gpu_hpnn_merge_golden.py: tests/golden/hpnn_merge_parent.npz.  Only the model's public call / backward, layers.Context.use_side and
ops.bc_ring_fwd / bc_ring_bwd with a flag are used, so the same file runs on any commit: the committed golden is the run of the commit BEFORE the
eight-branch merge moved into models._BottleneckMerge and the two ring kernel pairs became one, and the test holds the present code to it bit for bit.

    python tools/record_hpnn_merge_golden.py [out.npz]

The test imports `CASES`, `RING_SHAPES`, `run_model`, `run_ring` and `gradient_record` from here, so golden and test cannot drift apart in how a
case is run.

A gradient is stored in full if the file then stays below FILE_MAX (the largest golden committed before this one); otherwise as its SHA-256 plus one
float64 sum per parameter, so that a mismatch names the layer."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'hpnn_merge_parent.npz')
FILE_MAX = 733696                                   # tests/golden/smoother_parent.npz
N = 2

# name -> (H, W, model keywords over configs.hpnn_tiny(), branch streams on)
CASES = {
    # factors 2 and 4 divide the grid, 3, 8 and 16 do not: pyramid-fed branches beside ones that pool with SAME padding and add into d_initial on stream 0
    'dirichlet_36x40': (36, 40, dict(bc_type='dirichlet'), True),
    # every factor divides: 16 comes from 8, which comes from 4, which comes from 2
    'neumann_48x48': (48, 48, dict(bc_type='neumann'), True),
    'one_neumann_edge_enforce_36x40': (36, 40, dict(bc_type={'left': 'neumann'}, smoother_boundaries='enforce', postsmoother_iterations=2), True),
    'dirichlet_36x40_one_stream': (36, 40, dict(bc_type='dirichlet'), False),
}
RING_SHAPES = [(3, 3), (3, 5), (4, 4), (5, 7)]      # H = 3: the single interior row mirrors into both ring rows, three gather entries at once


def model_inputs(H, W):
    rng = np.random.default_rng([31, H, W])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(rng.uniform(-1, 1, (N, 1, H, W))), f32(rng.uniform(5e-3, 5e-2, (N, 1))), f32(rng.standard_normal((N, 1, H, W)))


def run_model(name, model_cfg=None):
    """One case on the GPU: forward (training) and one backward of the seeded dpred -> (prediction, {parameter: gradient})."""
    from oracle import hpnn as ohpnn
    from poisson_cnn_amd import configs
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    H, W, kw, streams = CASES[name]
    base = model_cfg or configs.hpnn_tiny()['model']
    model = Homogeneous_Poisson_NN_Legacy(**dict(base, **kw))
    model.set_weights(ohpnn.init_params(base, seed=5, gain=1.6, randomize_all=True))     # (no keyword of a case changes a weight's name or shape)
    if not streams:
        model.ctx.use_side = False
    rhs, dx, dpred = (torch.tensor(a, device='cuda') for a in model_inputs(H, W))
    pred = model.call([rhs, dx], training=True)
    model.backward(dpred)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), {n: model.store.g[n].cpu().numpy().copy() for n in model.store.trainable_names()}


def gradient_record(grads, full):
    flat = np.concatenate([g.ravel() for g in grads.values()])
    if full:
        return {'grad': flat}
    return {'grad_sha256': np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8),
            'grad_sums': np.array([g.astype(np.float64).sum() for g in grads.values()]),
            'grad_names': np.array(list(grads))}


def ring_inputs(H, W):
    rng = np.random.default_rng([37, H, W])
    return np.ascontiguousarray(rng.standard_normal((N, H, W, 1)), dtype=np.float32)


def run_ring(H, W, fwd, bwd, arg):
    """fwd / bwd: the ring operators under test; arg: their flag or mask."""
    x = torch.tensor(ring_inputs(H, W), device='cuda')
    return {'fwd': fwd(x, arg).cpu().numpy(), 'bwd': bwd(x, arg).cpu().numpy()}


def _collect(full):
    from poisson_cnn_amd import ops
    out = {}
    for name in CASES:
        pred, grads = run_model(name)
        out['model/%s/pred' % name] = pred
        out.update({'model/%s/%s' % (name, k): v for k, v in gradient_record(grads, full).items()})
    for H, W in RING_SHAPES:
        for flag in (0, 1):
            out.update({'ring/%dx%d/flag%d/%s' % (H, W, flag, k): v for k, v in run_ring(H, W, ops.bc_ring_fwd, ops.bc_ring_bwd, bool(flag)).items()})
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for full in (True, False):
        out = _collect(full)
        np.savez_compressed(path, **out)
        if os.path.getsize(path) < FILE_MAX:
            break
    print('wrote %s: %d arrays, %d bytes, gradients %s' % (path, len(out), os.path.getsize(path), 'in full' if full else 'as digest and per-parameter sums'))


if __name__ == '__main__':
    main()
