"""The handle-owned buffers (csrc/pcnn_host.h: pcnn_buffer / pcnn_reserve) shared between entry points, and the descriptor check
(pcnn_conv_desc_problem) in the entry points beside pcnn_conv2d_fwd.

Buffers: calls are interleaved on ONE handle so that each shared buffer is grown by another entry point than the one that uses it next; every result must
be bit-identical to the same call on a fresh handle (a stream of its own).  The byte counts in the comments are the launchers' own `need` formulas.

Refusals: pad_mode = 3, ldx = Cin - 1 and a REFLECT pad of H rows are refused on the host by pcnn_conv2d_wgrad, pcnn_grouped_conv2d_fwd and
pcnn_grouped_conv2d_wgrad: RuntimeError, nothing launched (the output keeps its canary), and the handle then completes a valid call."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_ops

pytestmark = pytest.mark.gpu
CANARY = -12345.0
TOL = 2e-6       # forward, rel-L2 against fp64 (tests/test_gpu_conv.py)
TOL_RED = 5e-6   # filter gradients: sums over all pixels (tests/test_gpu_grouped.py)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


class OnFreshHandle:
    """Runs its block on a new stream, i.e. on a libpcnn handle that has served no call yet, and destroys that handle afterwards."""

    def __enter__(self):
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        self.ctx = torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        from poisson_cnn_amd import ops
        self.stream.synchronize()
        self.ctx.__exit__(*exc)
        ops.release_stream_handle(self.stream.cuda_stream)
        return False


def run_interleaved(steps):
    """steps: (name, callable returning a tensor or a tuple of tensors).  All of them in order on one fresh handle, then each alone on a fresh handle."""
    def as_list(r):
        return [t.clone() for t in (r if isinstance(r, tuple) else (r,))]
    with OnFreshHandle():
        shared = [as_list(fn()) for _, fn in steps]
    for (name, fn), got in zip(steps, shared):
        with OnFreshHandle():
            alone = as_list(fn())
        torch.cuda.synchronize()
        for a, b in zip(got, alone):
            assert torch.isfinite(b).all() and bool((b != 0).any()), name
            assert torch.equal(a, b), '%s: differs from the same call on a fresh handle' % name


def test_filter_scratch_grown_between_its_users():
    from poisson_cnn_amd import ops
    g = torch.Generator(device='cuda').manual_seed(11)
    xs, ws = torch.randn(1, 16, 16, 4, device='cuda', generator=g), torch.randn(3, 3, 4, 4, device='cuda', generator=g)
    xl, wl = torch.randn(1, 24, 24, 64, device='cuda', generator=g), torch.randn(17, 17, 64, 64, device='cuda', generator=g) / 136
    pred, tgt = torch.randn(2, 1, 40, 40, device='cuda', generator=g), torch.randn(2, 1, 40, 40, device='cuda', generator=g)

    def narrow():            # 9 taps x 4 x 4 floats = 576 B: the 4 MiB floor
        return ops.conv2d_fwd(xs, ws, None, pad_top=1, pad_left=1, act='tanh')

    def direct():            # (289 x 64 + 64 + 16) x 2 x 32 x 4 B = 4 755 456 B > 4 MiB: grows
        return ops.conv2d_fwd(xl, wl, None, pad_top=8, pad_left=8)

    def loss():              # 2 x 64 x 4 floats of partial sums in the buffer the convolution grew
        return ops.loss_partials(pred, tgt, None)

    mode = ops.get_spectral_mode()
    ops.set_spectral_mode('off')
    try:
        run_interleaved([('narrow', narrow), ('direct 17 x 17', direct), ('loss_partials', loss), ('narrow again', narrow), ('direct again', direct)])
    finally:
        ops.set_spectral_mode(mode)


def test_auxiliary_scratch_grown_between_its_users():
    from poisson_cnn_amd import ops
    g = torch.Generator(device='cuda').manual_seed(12)
    x, gs, dy = torch.randn(2, 20, 20, 3, device='cuda', generator=g), torch.randn(2, device='cuda', generator=g), torch.randn(2, 20, 20, 3, device='cuda', generator=g)
    xr = torch.randn(2, 64, 64, 8, device='cuda', generator=g)
    N, H, W = 2, 512, 520
    u, rhs = torch.randn(N, H, W, 1, device='cuda', generator=g), torch.randn(N, H, W, 1, device='cuda', generator=g)
    coef = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0, 1.0, -0.25]] * N, device='cuda')
    sweeps = ops.jacobi_k_max(3, 3) + 1          # two launches: the intermediate image lives in the handle's buffer

    def scale_bwd():         # N x SS_SPLIT floats: the 1 MiB floor
        return ops.sample_scale_bwd(x, gs, dy)

    def resize():            # two-pass bilinear: N hc Wo C x 4 B = 2 x 64 x 512 x 8 x 4 = 2 097 152 B > 1 MiB: grows
        return ops.resize_fwd(xr, (128, 512), 'bilinear')

    def jacobi():            # N H W x 4 B = 2 129 920 B: grows again
        return ops.jacobi_fused(u, rhs, coef, (3, 3), sweeps)

    run_interleaved([('sample_scale_bwd', scale_bwd), ('resize_fwd', resize), ('jacobi_fused', jacobi), ('sample_scale_bwd again', scale_bwd), ('resize_fwd again', resize)])


# ------------------------------------------------------------------------------------------------------------------ refusals
N_, H_, W_, C_ = 2, 8, 8, 4
BAD = [('pad_mode', dict(pad_mode=3)), ('channel stride', dict(ldx=C_ - 1)), ('padding exceeds', dict(pad_mode=2, pad_top=H_))]


def _desc(**changes):
    from poisson_cnn_amd import ops
    d = ops.conv_desc((N_, H_, W_, C_), C_, (3, 3, C_, C_), (H_, W_), C_, 1, 1)
    for k, v in changes.items():
        setattr(d, k, v)
    return d


def _problem():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N_, C_, H_, W_)).astype(np.float32)
    dz = rng.standard_normal((N_, C_, H_, W_)).astype(np.float32)
    w = (rng.standard_normal((N_, 3, 3, C_, C_)) / 6).astype(np.float32)             # one filter per sample (the ordinary calls use w[0])
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    dw = np.zeros((N_, 3, 3, C_, C_))                                                 # per-sample filter gradients of the zero-padded convolution
    for i in range(3):
        for j in range(3):
            dw[:, i, j] = np.einsum('ncyx,noyx->nco', xp[:, :, i:i + H_, j:j + W_], dz.astype(np.float64))
    dev = lambda a: torch.tensor(np.ascontiguousarray(a.transpose(0, 2, 3, 1)), device='cuda')
    return x, dz, w, dw, dev(x), dev(dz)


@pytest.mark.parametrize('text,changes', BAD)
def test_conv2d_wgrad_refuses_a_bad_descriptor_on_the_host(text, changes):
    from poisson_cnn_amd import ops
    x, dz, w, dw_ref, xd, dzd = _problem()
    d = _desc()
    ws = torch.empty(ops._lib.load().pcnn_conv2d_wgrad_workspace(ctypes.byref(d)) // 4 + 16, device='cuda')
    dw = torch.full((3, 3, C_, C_), CANARY, device='cuda')
    h = ops.handle()
    with pytest.raises(RuntimeError, match=text):
        h.call('pcnn_conv2d_wgrad', ctypes.byref(_desc(**changes)), ops._p(xd), ops._p(dzd), ops._p(dw), ops._p(ws), ctypes.c_size_t(ws.numel() * 4))
    torch.cuda.synchronize()
    assert bool((dw == CANARY).all())
    h.call('pcnn_conv2d_wgrad', ctypes.byref(d), ops._p(xd), ops._p(dzd), ops._p(dw), ops._p(ws), ctypes.c_size_t(ws.numel() * 4))
    assert rel(dw.cpu().numpy(), dw_ref.sum(axis=0)) < TOL_RED


@pytest.mark.parametrize('text,changes', BAD)
def test_grouped_conv2d_fwd_refuses_a_bad_descriptor_on_the_host(text, changes):
    from poisson_cnn_amd import ops
    x, dz, w, dw_ref, xd, dzd = _problem()
    wd = torch.tensor(w.reshape(N_, -1), device='cuda')
    y = torch.full((N_, H_, W_, C_), CANARY, device='cuda')
    args = (ops._p(xd), ops._p(wd), ctypes.c_longlong(wd.stride(0)), ops._p(None), ctypes.c_longlong(0), ctypes.c_int(0), ops._p(y))
    h = ops.handle()
    with pytest.raises(RuntimeError, match=text):
        h.call('pcnn_grouped_conv2d_fwd', ctypes.byref(_desc(**changes)), *args)
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())
    h.call('pcnn_grouped_conv2d_fwd', ctypes.byref(_desc()), *args)
    for n in range(N_):
        ref = np_ops.padded_conv2d(x[n:n + 1].astype(np.float64), w[n].astype(np.float64), None, 'CONSTANT', 0.0, 'linear')
        assert rel(y[n:n + 1].cpu().numpy().transpose(0, 3, 1, 2), ref) < TOL


@pytest.mark.parametrize('text,changes', BAD)
def test_grouped_conv2d_wgrad_refuses_a_bad_descriptor_on_the_host(text, changes):
    from poisson_cnn_amd import ops
    x, dz, w, dw_ref, xd, dzd = _problem()
    d = _desc()
    lib = ops._lib.load()
    lib.pcnn_grouped_conv2d_wgrad_workspace.restype = ctypes.c_size_t
    ws = torch.empty(lib.pcnn_grouped_conv2d_wgrad_workspace(ctypes.byref(d)) // 4 + 16, device='cuda')
    dw = torch.full((N_, 3 * 3 * C_ * C_), CANARY, device='cuda')
    args = (ops._p(xd), ops._p(dzd), ops._p(dw), ctypes.c_longlong(dw.stride(0)), ops._p(ws))
    h = ops.handle()
    with pytest.raises(RuntimeError, match=text):
        h.call('pcnn_grouped_conv2d_wgrad', ctypes.byref(_desc(**changes)), *args)
    torch.cuda.synchronize()
    assert bool((dw == CANARY).all())
    h.call('pcnn_grouped_conv2d_wgrad', ctypes.byref(d), *args)
    assert rel(dw.cpu().numpy().reshape(dw_ref.shape), dw_ref) < TOL_RED
