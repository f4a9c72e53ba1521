"""Geometry-general fp64 reference of the fused pad + convolution (include/pcnn.h pcnn_conv_desc), shared by
tests/test_conv_geometry_reference.py (CPU: pins this module against numpy.pad + torch conv2d) and tests/test_gpu_conv_geometry.py (the
kernels).  The descriptor's meaning, followed literally: output (oy, ox) reads padded input rows oy - pad_top + ty, ty = 0 .. kh - 1, and
columns ox - pad_left + tx; the bottom / right pads are what Ho, Wo imply.  Layout here: x (N, C, H, W), w HWIO (kh, kw, Cin, Cout)."""
import numpy as np
import torch

from oracle import np_ops, torch_twin

U = 2.0 ** -24                      # unit roundoff of fp32


def pads_of(H, W, kh, kw, pad_top, pad_left, out_hw):
    """((pad_top, pb), (pad_left, pr)) with pb = Ho - 1 - pad_top + kh - 1 - (H - 1), the same in x (csrc/conv_fwd.hip states it the same way)."""
    Ho, Wo = out_hw
    pb = Ho - 1 - pad_top + kh - 1 - (H - 1)
    pr = Wo - 1 - pad_left + kw - 1 - (W - 1)
    if pb < 0 or pr < 0:
        raise ValueError('negative bottom / right pad (%d, %d): the output does not reach the image edge' % (pb, pr))
    return (pad_top, pb), (pad_left, pr)


def ref_conv(x, w, bias, pad_top, pad_left, out_hw, mode='CONSTANT', value=0.0, act='linear'):
    """fp64 numpy: pad2d (raises beyond what tf.pad allows) + VALID cross-correlation + bias + activation -> (N, Cout, Ho, Wo)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    kh, kw = w.shape[:2]
    pads = pads_of(x.shape[2], x.shape[3], kh, kw, pad_top, pad_left, out_hw)
    y = np_ops.conv2d_valid(np_ops.pad2d(x, pads, mode, value), w, None if bias is None else np.asarray(bias, dtype=np.float64))
    assert y.shape[2:] == tuple(out_hw), (y.shape, out_hw)
    return np_ops.activation(y, act)


def twin_conv(x, w, bias, pad_top, pad_left, out_hw, mode='CONSTANT', value=0.0, act='linear'):
    """The same on fp64 torch tensors (differentiable)."""
    kh, kw = w.shape[:2]
    pads = pads_of(x.shape[2], x.shape[3], kh, kw, pad_top, pad_left, out_hw)
    for (a, b), n in zip(pads, x.shape[2:]):                     # the twin's index map does not refuse these itself
        lim = n if mode.upper() == 'SYMMETRIC' else n - 1
        if mode.upper() != 'CONSTANT' and (a > lim or b > lim):
            raise ValueError('pad %s exceeds what tf.pad %s allows for size %d' % ((a, b), mode, n))
    y = torch_twin.conv2d_valid(torch_twin.pad2d(x, pads, mode, value), w, bias)
    return torch_twin.activation(y, act)


def gradients(x, w, bias, dz, pad_top, pad_left, mode='CONSTANT', value=0.0, act='linear'):
    """(dx, dw, dbias) of L = <twin_conv(x, w, bias), dz> by fp64 autograd, as numpy arrays (dbias None without a bias)."""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    bt = None if bias is None else torch.tensor(np.asarray(bias, dtype=np.float64), requires_grad=True)
    dzt = torch.tensor(np.asarray(dz, dtype=np.float64))
    y = twin_conv(xt, wt, bt, pad_top, pad_left, tuple(dzt.shape[2:]), mode, value, act)
    (y * dzt).sum().backward()
    return xt.grad.numpy(), wt.grad.numpy(), None if bt is None else bt.grad.numpy()


def regions(y, kh, kw):
    """[(name, view)] of an (N, C, Ho, Wo) array: the whole tensor, the border band (outer kh - 1 rows and kw - 1 columns, as a copy with the
    interior zeroed - the interior then adds nothing to either norm), each output channel, each sample.  Apply the same call to the result and
    to the reference."""
    y = np.asarray(y)
    N, C, Ho, Wo = y.shape
    out = [('whole', y)]
    by, bx = min(kh - 1, Ho), min(kw - 1, Wo)
    if by or bx:
        band = y.copy()
        if Ho > 2 * by and Wo > 2 * bx:
            band[:, :, by:Ho - by, bx:Wo - bx] = 0
        out.append(('border', band))
    out += [('channel %d' % c, y[:, c]) for c in range(C)]
    out += [('sample %d' % n, y[n]) for n in range(N)]
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst_region(got, ref, kh, kw):
    """(name, rel-L2) of the region where `got` is farthest from `ref`."""
    return max(((n, rel(g, r)) for (n, g), (_, r) in zip(regions(got, kh, kw), regions(ref, kh, kw))), key=lambda t: t[1])


def gamma(K):
    """K u / (1 - K u), u = 2^-24: |fl(sum of K products) - exact| <= gamma(K) sum |products| for ANY order of an fp32 evaluation
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); fused multiply-adds only lower the count."""
    return K * U / (1.0 - K * U)
