"""fp64 torch twin of the UNet baseline, written from the reference's layer sequence (models/UNet.py:212-267), for the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_twin as T


def conv_same(x, w, b):
    k = w.shape[0]
    return F.conv2d(x, w.permute(3, 2, 0, 1), b, padding=k // 2)


def maxpool_same(x, p):
    H, W = x.shape[2:]
    th, tw = (-(-H // p)) * p - H, (-(-W // p)) * p - W
    x = F.pad(x, (tw // 2, tw - tw // 2, th // 2, th - th // 2), value=-float('inf'))
    return F.max_pool2d(x, p)


def mask_nchw(shape_nchw, rate, seed, lid):
    from poisson_cnn_amd import ops
    N, C, H, W = shape_nchw
    m = ops.dropout_keep_mask((N, H, W, C), rate, seed, lid)
    return torch.from_numpy(np.ascontiguousarray(m.transpose(0, 3, 1, 2)))


def forward(model, P, x, drop=None):
    """P: name -> fp64 torch tensor (may require grad); x (N, Cin, H, W) fp64; drop = (rate, seed) applies the ConvBlock dropout."""
    act = torch.relu
    lid = [0]

    def conv_act(spec, t):
        z = conv_same(t, P[spec[0]], P[spec[1]])
        if drop is not None:
            z = z * mask_nchw(z.shape, drop[0], drop[1], lid[0]).to(z.dtype) / (1.0 - drop[0])
        lid[0] += 1
        return act(z)

    skips = []
    t = x
    for c1, c2 in model.down:
        t = conv_act(c2, conv_act(c1, t))
        skips.append(t)
        t = maxpool_same(t, model.pool)
    t = conv_act(model.bottom[1], conv_act(model.bottom[0], t))
    for j, ((dk, db, _, _), (c1, c2)) in enumerate(model.up):
        s = skips[len(skips) - 1 - j]
        u = T.conv2d_transpose_same(t, P[dk], P[db], tuple(s.shape[2:]), model.pool, 'relu')
        t = conv_act(c2, conv_act(c1, torch.cat([s, u], 1)))
    return act(conv_same(t, P[model.head[0]], P[model.head[1]]))


def params(model, requires_grad=False):
    return {n: torch.from_numpy(w.astype(np.float64)).requires_grad_(requires_grad) for n, w in zip(model.weight_names, model.get_weights())}
