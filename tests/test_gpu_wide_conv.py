"""Wide-channel convolution kernels (csrc/conv_wide.hip, the UNet baseline) against fp64 torch CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_twin as T
from poisson_cnn_amd import ops

pytestmark = pytest.mark.gpu

UNET_PAIRS = [(1, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 256), (256, 128), (128, 64),
              (1024, 512)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def nchw(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def ref_conv(x, w, b):
    return F.conv2d(nchw(x), w.double().cpu().permute(3, 2, 0, 1), None if b is None else b.double().cpu(), padding=w.shape[0] // 2)


def case(N, H, W, ci, co, k, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(N, H, W, ci, device='cuda', generator=g)
    w = torch.randn(k, k, ci, co, device='cuda', generator=g) / np.sqrt(k * k * ci)
    b = torch.randn(co, device='cuda', generator=g)
    return x, w, b


def spatial(ci, co):
    return (1, 6, 7) if max(ci, co) >= 1024 else ((1, 9, 11) if max(ci, co) >= 512 else (2, 13, 15))


@pytest.mark.parametrize('ci,co', UNET_PAIRS + [(64, 1), (1, 12), (12, 40), (40, 1), (40, 12), (12, 12)])
def test_forward_dgrad_wgrad(ci, co):
    k = 1 if co == 1 and ci == 64 else 3
    N, H, W = spatial(ci, co) if (ci, co) in UNET_PAIRS else (2, 37, 45)
    x, w, b = case(N, H, W, ci, co, k, ci * 1000 + co)
    y = ops.wide_conv2d_fwd(x, w, b, act='relu')
    yr = torch.relu(ref_conv(x, w, b))
    assert rel(nchw(y), yr) <= 2e-6
    # data gradient with the producer's ReLU' taken from its output a (here: x through a ReLU)
    a = torch.relu(x)
    dz = torch.randn(N, H, W, co, device='cuda') + 0.3            # non-zero mean: dbias is then a well-conditioned sum
    dx = ops.wide_conv2d_dgrad(dz, ops.flip_transpose_weights(w), act_out=a, act='relu')
    xr = nchw(x).requires_grad_(True)
    F.conv2d(xr, w.double().cpu().permute(3, 2, 0, 1), padding=k // 2).mul(nchw(dz)).sum().backward()
    dxr = xr.grad * (nchw(a) > 0)
    assert rel(nchw(dx), dxr) <= 2e-6
    # filter + bias gradient, deterministic
    dw = torch.empty_like(w)
    db = torch.empty(co, device='cuda')
    ops.wide_conv2d_wgrad(x, dz, w.shape, dw=dw, dbias=db)
    wr = w.double().cpu().permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    F.conv2d(nchw(x), wr, padding=k // 2).mul(nchw(dz)).sum().backward()
    assert rel(dw.permute(3, 2, 0, 1), wr.grad) <= 5e-6
    assert rel(db, nchw(dz).sum((0, 2, 3))) <= 5e-6
    dw2, db2 = torch.empty_like(w), torch.empty(co, device='cuda')
    ops.wide_conv2d_wgrad(x, dz, w.shape, dw=dw2, dbias=db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('k', [1, 5, 7])
def test_kernel_sizes_and_odd_tails(k):
    x, w, b = case(2, 37, 45, 12, 40, k, k)
    y = ops.wide_conv2d_fwd(x, w, b, act='tanh')
    assert rel(nchw(y), torch.tanh(ref_conv(x, w, b))) <= 2e-6


def test_channel_slices_and_accumulate():
    x, w, b = case(2, 11, 13, 40, 24, 3, 5)
    big = torch.full((2, 11, 13, 70), 7.0, device='cuda')
    xin = torch.zeros(2, 11, 13, 48, device='cuda')
    xin[..., 3:43] = x
    ops.wide_conv2d_fwd(xin[..., 3:43], w, b, out=big[..., 30:54])
    assert rel(nchw(big[..., 30:54]), ref_conv(x, w, b)) <= 2e-6
    assert (big[..., :30] == 7).all() and (big[..., 54:] == 7).all()
    dz = torch.randn(2, 11, 13, 24, device='cuda')
    base = torch.randn(2, 11, 13, 40, device='cuda')
    acc = base.clone()
    ops.wide_conv2d_dgrad(dz, ops.flip_transpose_weights(w), out=acc, accumulate=True)
    plain = ops.wide_conv2d_dgrad(dz, ops.flip_transpose_weights(w))
    assert rel(acc, base + plain) <= 1e-7


@pytest.mark.parametrize('f,ci,co,H,W', [(2, 512, 256, 24, 26), (2, 128, 64, 37, 45), (3, 40, 12, 22, 25), (3, 12, 40, 24, 27), (2, 16, 8, 97, 101)])
@pytest.mark.parametrize('act', ['relu', 'linear'])
def test_deconv(f, ci, co, H, W, act):
    hc, wc = -(-H // f), -(-W // f)
    g = torch.Generator(device='cuda').manual_seed(f * 100 + ci)
    x = torch.randn(2, hc, wc, ci, device='cuda', generator=g)
    k = torch.randn(f, f, co, ci, device='cuda', generator=g) / np.sqrt(ci)
    b = torch.randn(co, device='cuda', generator=g)
    y = ops.wide_deconv_fwd(x, k, b, (H, W), f, act=act)
    xr = nchw(x).requires_grad_(True)
    kr = k.double().cpu().requires_grad_(True)
    yr = T.conv2d_transpose_same(xr, kr, b.double().cpu(), (H, W), f, act)
    assert rel(nchw(y), yr) <= 2e-6
    dy = torch.randn(2, H, W, co, device='cuda')
    dz = dy * (y > 0) if act == 'relu' else dy
    yr.mul(nchw(dy)).sum().backward()
    a = torch.relu(torch.randn(2, hc, wc, ci, device='cuda'))
    dx = ops.wide_deconv_bwd_data(dz, k, (hc, wc), f, act_out=a, act='relu')
    assert rel(nchw(dx), xr.grad * (nchw(a) > 0)) <= 2e-6
    dk = ops.wide_deconv_bwd_filter(x, dz, f)
    assert rel(dk, kr.grad) <= 5e-6
    assert torch.equal(dk, ops.wide_deconv_bwd_filter(x, dz, f))


def test_dropout_forward_and_backward():
    rate, seed, lid = 0.5, 1234, 5
    x, w, b = case(2, 21, 23, 24, 72, 3, 9)
    y = ops.wide_conv2d_fwd(x, w, b, act='relu', dropout=(rate, seed, lid))
    keep = torch.from_numpy(ops.dropout_keep_mask((2, 21, 23, 72), rate, seed, lid))
    z = ref_conv(x, w, b).permute(0, 2, 3, 1)
    yr = torch.relu(z * keep / (1 - rate))
    assert rel(y, yr) <= 2e-6
    assert abs(1 - keep.double().mean().item() - rate) < 0.02
    # linear activation: the backward regenerates the mask from the hash
    yl = ops.wide_conv2d_fwd(x, w, b, act='linear', dropout=(rate, seed, lid))
    assert rel(yl, z * keep / (1 - rate)) <= 2e-6
    w2 = torch.randn(3, 3, 72, 8, device='cuda') * 0.1
    dz = torch.randn(2, 21, 23, 8, device='cuda')
    for act, out in (('relu', y), ('linear', yl)):
        dx = ops.wide_conv2d_dgrad(dz, ops.flip_transpose_weights(w2), act_out=out, act=act, dropout=(rate, seed, lid))
        ar = ref_conv(x, w, b).requires_grad_(True)
        t = ar * keep.permute(0, 3, 1, 2) / (1 - rate)
        t = torch.relu(t) if act == 'relu' else t
        F.conv2d(t, w2.double().cpu().permute(3, 2, 0, 1), padding=1).mul(nchw(dz)).sum().backward()
        assert rel(nchw(dx), ar.grad) <= 2e-6, act
