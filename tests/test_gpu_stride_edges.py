"""The row, reduction and element-wise kernels past one trip of their strided loops, one block of their grids and one partial sum per sample: softmax,
LayerNormalization, Dense, the pyramid pools, the loss partials and their backward, set_max_magnitude, the optimizer / axpby grid-stride wrap and the
multi-block scale gradients - each against the same formula evaluated in float64 by the functions below.

Bounds.  Where another test of the same op has a bound it is used here (TOL / TOL_RED of tests/test_gpu_ops.py, 1e-6 / 1e-5 for softmax, 1e-6 / 2e-6 for
set_max_magnitude).  Every wider bound is 4 x the rel-L2 error of the SAME formula function below evaluated in float32 by NumPy on the CPU on the test's own
inputs (4 x because the order of the sums differs); the measured figure stands beside the bound.  The reference functions work in the precision of their
arguments, so `_layernorm(*(a.astype(np.float32) for a in args))` is that float32 evaluation."""
import numpy as np
import pytest
import torch

from oracle import np_ops

pytestmark = pytest.mark.gpu
TOL = 2e-6      # per-op rel-L2 (fp32 kernels vs fp64), as in tests/test_gpu_ops.py
TOL_RED = 5e-6  # long fp32 reductions, as in tests/test_gpu_ops.py
GRID_CAP = 8192 * 256   # threads of the capped grid of the element-wise kernels (csrc/pointwise.hip grid1d)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device='cuda')


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ----------------------------------------------------------------------------- 1. softmax (one 64-lane wave per row, f += 64)
SOFTMAX_F = [1, 2, 63, 64, 65, 129, 1000]


def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _softmax_bwd(y, dy):
    return y * (dy - (dy * y).sum(1, keepdims=True))


def softmax_inputs(F):
    """x, the same rows shifted by +80 / -80 / +80, and dy.  x is the shifted matrix minus its offset, so both are float32 numbers that differ by exactly 80."""
    rng = np.random.default_rng(100 + F)
    off = np.array([80.0, -80.0, 80.0])[:, None]
    shifted = f32(3 * rng.standard_normal((3, F)) + off)
    return shifted - off, shifted, f32(rng.standard_normal((3, F)))


@pytest.mark.parametrize('F', SOFTMAX_F)
def test_softmax_rows_of_one_to_sixteen_trips(F):
    """F = 1, 2 (idle lanes), 63 / 64 / 65 (the end of the first trip), 129 (a third trip of one lane), 1000; a row offset of +-80 (exp overflows unless the row
    maximum is subtracted); -inf entries (exactly 0, no NaN); the backward y (dy - sum dy y) on the kernel's own y."""
    from poisson_cnn_amd import ops
    x, shifted, dy = softmax_inputs(F)
    assert np.array_equal(f32(x), x) and np.array_equal(f32(shifted), shifted)
    ref = _softmax(x)
    y = ops.softmax_fwd(dev(x))
    assert rel(host(y), ref) < 1e-6
    assert np.abs(host(y).sum(1) - 1.0).max() < 1e-6              # float32 on the CPU: <= 1.1e-7 at every F
    assert rel(host(ops.softmax_fwd(dev(shifted))), ref) < 1e-6
    dx = ops.softmax_bwd(y, dev(dy))
    assert rel(host(dx), _softmax_bwd(host(y), dy)) < 1e-5
    if F > 1:
        holes = sorted({F - 1, F // 2, 0} - {int(np.argmax(x[1]))})[:F - 1]
        xi = x.copy()
        xi[1, holes] = -np.inf
        yi = host(ops.softmax_fwd(dev(xi)))
        assert np.isfinite(yi).all() and (yi[1, holes] == 0.0).all()
        assert np.abs(yi.sum(1) - 1.0).max() < 1e-6 and rel(yi, _softmax(xi)) < 1e-6


# ----------------------------------------------------------------------------- 2. LayerNormalization (256 threads per row; params: cdiv(F, 256) blocks)
LN_EPS = float(np.float32(1e-3))
LN_F = [1, 2, 255, 256, 257, 10816]         # 10816 = 13 x 13 x 8 x 8, the hyper-network row the layer normalises
# Measured rel-L2 error of _layernorm / _layernorm_bwd in float32 on these inputs, (kind, N, F) -> quantity -> figure, wherever it is above TOL / 4; the bound of
# that quantity is 4 x the figure, every other bound is TOL.  Three causes.  The float32 mean of a row around 100 is off by up to half an ulp of 100 (3.8e-6), a
# shift of every x - mean that no float32 evaluation avoids: y and dgamma of the 'offset' input.  At F = 2 xhat is +-1 up to epsilon / variance, so dx is the small
# remainder of g - mean(g) - xhat mean(g xhat): 2.4e-5 even at unit scale and 1.3e-3 where the mean of 100 + a, 100 + b is not a float32 number.  The mean of 257
# unit normals of the one-row case is 3e-4 of their size, so its relative error is that much larger.  F = 1 is exact and is checked as such.
LN_MEASURED = {
    ('unit', 1, 2): {'dx': 8.34e-6}, ('unit', 5, 2): {'dx': 2.39e-5}, ('unit', 1, 257): {'mean': 3.41e-4},
    ('offset', 1, 2): {'dx': 6.30e-6}, ('offset', 5, 2): {'y': 5.95e-6, 'dx': 1.30e-3, 'dgamma': 1.92e-5},
    ('offset', 1, 255): {'y': 6.26e-6, 'dx': 8.10e-7, 'dgamma': 8.71e-6}, ('offset', 5, 255): {'y': 2.46e-6, 'dgamma': 3.24e-6},
    ('offset', 1, 256): {'y': 8.36e-6, 'dgamma': 1.13e-5}, ('offset', 5, 256): {'y': 1.48e-6, 'dgamma': 1.74e-6},
    ('offset', 1, 257): {'y': 6.58e-6, 'dx': 6.76e-7, 'dgamma': 9.40e-6}, ('offset', 5, 257): {'y': 4.50e-6, 'dx': 7.45e-7, 'dgamma': 6.39e-6},
    ('offset', 1, 10816): {'y': 2.55e-6, 'dgamma': 3.54e-6}, ('offset', 5, 10816): {'y': 4.27e-6, 'dgamma': 5.96e-6},
}


def _layernorm(x, gamma, beta, eps):
    mean = x.mean(1, keepdims=True)
    rstd = 1 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + eps)
    return (x - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def _layernorm_bwd(x, gamma, eps, dy):
    """(dx, dgamma, dbeta) of sum(dy * layernorm(x))."""
    mean = x.mean(1, keepdims=True)
    rstd = 1 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + eps)
    xh, g = (x - mean) * rstd, dy * gamma
    dx = rstd * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def layernorm_inputs(N, F, kind):
    rng = np.random.default_rng(1000 * N + F + (7 if kind == 'offset' else 0))
    x = f32(rng.standard_normal((N, F)) + (100.0 if kind == 'offset' else 0.0))
    return x, f32(rng.uniform(0.5, 1.5, F)), f32(rng.standard_normal(F)), f32(rng.standard_normal((N, F)))


@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('F', LN_F)
def test_layernorm_rows_past_one_trip_and_one_params_block(N, F):
    """Forward (y, saved mean and rstd) and backward (dx, dgamma, dbeta) at F = 1, 2, around 256 and at 10816 (43 trips, 43 parameter blocks); dgamma / dbeta
    are overwritten, not accumulated; at F = 1 the row is its own mean: y == beta and dx == 0 exactly.

    The bound of dx at [F = 2, N = 1], unit input, is the one that made the backward form its row statistics in double: with the float32 rstd of the forward
    it measured 4.52e-5 against 3.34e-5."""
    from poisson_cnn_amd import ops
    for kind in ('unit', 'offset'):
        x, gamma, beta, dy = layernorm_inputs(N, F, kind)
        ry, rmean, rrstd = _layernorm(x, gamma, beta, LN_EPS)
        rdx, rdg, rdb = _layernorm_bwd(x, gamma, LN_EPS, dy)
        y, st = ops.layernorm_fwd(dev(x), dev(gamma), dev(beta), eps=LN_EPS)
        dgamma, dbeta = torch.full((F,), 1e30, device='cuda'), torch.full((F,), -7.0, device='cuda')
        dx = ops.layernorm_bwd(dev(x), dev(gamma), st, dev(dy), dgamma, dbeta, eps=LN_EPS)
        got = [host(t) for t in (y, st[0], st[1], dx, dgamma, dbeta)]
        for name, g, r in zip(('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta'), got, (ry, rmean, rrstd, rdx, rdg, rdb)):
            bound = max(TOL, 4 * LN_MEASURED.get((kind, N, F), {}).get(name, 0.0))
            assert rel(g, r) < bound, (kind, name, rel(g, r), bound)
        if F == 1:
            assert np.array_equal(got[0], np.broadcast_to(beta, (N, 1))) and not got[3].any()


# ----------------------------------------------------------------------------- 3. Dense
DENSE_SHAPES = [(1, 1, 1), (3, 7, 63), (4, 9, 64), (4, 9, 65), (5, 38, 10816), (70, 64, 5)]
DENSE_ACTS = ['linear', 'leaky_relu', 'tanh', 'relu']          # what layers.Dense takes besides softmax
LEAKY = float(np.float32(0.2))


def _act(z, act):
    return {'linear': lambda: z, 'leaky_relu': lambda: np.where(z > 0, z, LEAKY * z), 'tanh': lambda: np.tanh(z), 'relu': lambda: np.where(z > 0, z, 0 * z)}[act]()


def _dense(x, w, b, act):
    return _act(x @ w + (b if b is not None else 0), act)


def _dense_bwd(x, w, y, dy, act):
    """(dx, dw, db) from the layer's OUTPUT y, as the kernel forms them."""
    one = np.ones_like(y)
    dz = dy * {'linear': lambda: one, 'leaky_relu': lambda: np.where(y > 0, one, LEAKY * one), 'tanh': lambda: 1 - y * y, 'relu': lambda: np.where(y > 0, one, 0 * one)}[act]()
    return dz @ w.T, x.T @ dz, dz.sum(0)


def dense_inputs(N, In, Out):
    rng = np.random.default_rng(N + 10 * In + Out)
    return (f32(rng.standard_normal((N, In))), f32(rng.standard_normal((In, Out)) / np.sqrt(In)), f32(rng.standard_normal(Out)),
            f32(rng.standard_normal((N, Out))), f32(rng.standard_normal((In, Out))), f32(rng.standard_normal(Out)))


# float32 on the CPU: forward <= 8.9e-8, dx <= 4.2e-7 (the sums over 10816 outputs), dw <= 1.9e-7, db <= 3.0e-7 over all shapes and activations: below TOL / 4, so TOL holds
@pytest.mark.parametrize('act', DENSE_ACTS)
@pytest.mark.parametrize('N,In,Out', DENSE_SHAPES)
def test_dense_shapes_around_the_wave_and_the_wave_loop(N, In, Out, act):
    """Out = 1 / 63 / 64 / 65 around the 64 lanes that stride over the outputs, Out = 10816 (169 trips), N In = 4480 > the 4096 waves of the capped grid;
    dw and db accumulate into what they hold; no bias, no bias gradient, no dx."""
    from poisson_cnn_amd import ops
    x, w, b, dy, dw0, db0 = dense_inputs(N, In, Out)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    y = ops.dense_fwd(xd, wd, dev(b), act)
    assert rel(host(y), _dense(x, w, b, act)) < TOL
    rdx, rdw, rdb = _dense_bwd(x, w, host(y), dy, act)
    dw, db = ops.zeros((In, Out)), ops.zeros((Out,))
    dx = ops.dense_bwd(xd, wd, y, dyd, act, dw, db)
    assert tuple(dx.shape) == (N, In)
    assert rel(host(dx), rdx) < TOL and rel(host(dw), rdw) < TOL and rel(host(db), rdb) < TOL
    dw, db = dev(dw0), dev(db0)                                  # non-zero buffers come back as old + gradient
    dx = ops.dense_bwd(xd, wd, y, dyd, act, dw, db)
    assert rel(host(dx), rdx) < TOL and rel(host(dw), dw0 + rdw) < TOL and rel(host(db), db0 + rdb) < TOL
    yn = ops.dense_fwd(xd, wd, None, act)                        # use_bias=False: b = NULL, db = NULL
    assert rel(host(yn), _dense(x, w, None, act)) < TOL
    ndx, ndw, _ = _dense_bwd(x, w, host(yn), dy, act)
    dw = ops.zeros((In, Out))
    dx = ops.dense_bwd(xd, wd, yn, dyd, act, dw, None)
    assert rel(host(dx), ndx) < TOL and rel(host(dw), ndw) < TOL
    dw, db = ops.zeros((In, Out)), ops.zeros((Out,))             # the first layer of a network: dx = NULL
    assert ops.dense_bwd(xd, wd, y, dyd, act, dw, db, need_dx=False) is None
    assert rel(host(dw), rdw) < TOL and rel(host(db), rdb) < TOL


# ----------------------------------------------------------------------------- 4. pyramid pools (256 threads per bin, e += 256, LDS tree)
SPP_LEVELS = [1, 2, [3, 5]]


def spp_bins(H, W):
    bins = []
    for lv in SPP_LEVELS:
        lv = [lv, lv] if isinstance(lv, int) else lv
        iy, ix = np_ops.split_indices(H, lv[0]), np_ops.split_indices(W, lv[1])
        bins += [[iy[a], iy[a + 1], ix[c], ix[c + 1]] for a in range(lv[0]) for c in range(lv[1])]
    return np.array(bins, dtype=np.int32)


def _spp_max(x, bins):
    """Per sample and bin: the maximum over the bin's pixels and channels of an NHWC tensor and the LOWEST flat index (y W + x) C + c that holds it."""
    N, H, W, C = x.shape
    flat = np.arange(H * W * C).reshape(H, W, C)
    out, arg = np.empty((N, len(bins)), x.dtype), np.empty((N, len(bins)), np.int64)
    for b, (y0, y1, x0, x1) in enumerate(bins):
        ids = flat[y0:y1, x0:x1].ravel()                         # ascending, so argmax's first hit is the lowest flat index
        for n in range(N):
            k = np.argmax(x[n, y0:y1, x0:x1].ravel())
            out[n, b], arg[n, b] = x[n].ravel()[ids[k]], ids[k]
    return out, arg


def _spp_max_bwd(arg, dout, shape):
    dx = np.zeros((shape[0], int(np.prod(shape[1:]))), dout.dtype)
    for n in range(shape[0]):
        np.add.at(dx[n], arg[n], dout[n])
    return dx.reshape(shape)


def _spp_avg(x, bins):
    return np.stack([x[:, y0:y1, x0:x1].reshape(x.shape[0], -1).mean(1) for y0, y1, x0, x1 in bins], 1)


def _spp_avg_bwd(bins, dout, shape):
    dx = np.zeros(shape, dout.dtype)
    for b, (y0, y1, x0, x1) in enumerate(bins):
        dx[:, y0:y1, x0:x1] += (dout[:, b] / ((y1 - y0) * (x1 - x0) * shape[3]))[:, None, None, None]
    return dx


def spp_inputs(C=4):
    rng = np.random.default_rng(44 + C)
    shape = (2, 40, 44, C)
    return f32(rng.standard_normal(shape) + 1.0), f32(rng.standard_normal((2, 20))), spp_bins(40, 44)


def test_spp_max_bins_of_up_to_7040_elements():
    """The level-1 bin holds 40 x 44 x 4 = 7040 elements: 28 trips of the 256 threads.  Values and argmax exact, backward against float64."""
    from poisson_cnn_amd import ops
    x, dout, bins = spp_inputs()
    rout, rarg = _spp_max(x, bins)
    out, arg = ops.spp_max_fwd(dev(x), torch.tensor(bins, device='cuda'))
    assert np.array_equal(host(out), rout) and np.array_equal(arg.cpu().numpy(), rarg)
    assert rel(host(ops.spp_max_bwd(arg, dev(dout), x.shape)), _spp_max_bwd(rarg, dout, x.shape)) < TOL


def test_spp_max_sends_a_tied_bin_to_its_lowest_flat_index():
    """The tie rule of spp_max: the maximum's value is exact, its argmax is the LOWEST flat index among the tied elements and the backward sends the bin's whole
    gradient to that one element.  tf.reduce_max, which the reference's SpatialPyramidPool uses, splits the gradient evenly over the tied elements instead (as
    set_max_magnitude_bwd does here); torch's .max(dim).values, which the oracle's twin uses, is single-index like the kernel.  The two rules differ only on
    exact float ties inside a bin; this test pins the kernel's rule, it does not endorse it over the reference's.
    The same maximum sits at flat indices e, e + 1 and e + 3 x 256 of sample 0 with e odd: e and e + 3 x 256 fall to one thread on different trips, e + 1 to
    its even neighbour, which is the one the last step of the LDS tree keeps unless the index comparison is made.  Sample 1 puts the lowest index on thread 6."""
    from poisson_cnn_amd import ops
    x, dout, bins = spp_inputs()
    e, top = 1001, f32(np.abs(x).max() + 1.0)
    x[0].reshape(-1)[[e, e + 1, e + 768]] = top                  # threads 233 (trip 3), 234 and 233 again (trip 6)
    x[1].reshape(-1)[[e + 29, e + 768, e + 769]] = top           # threads 6 (the lowest index, which the tree meets from its odd side), 233 and 234
    rout, rarg = _spp_max(x, bins)
    assert rarg[0, 0] == e and rarg[1, 0] == e + 29
    out, arg = ops.spp_max_fwd(dev(x), torch.tensor(bins, device='cuda'))
    assert np.array_equal(host(out), rout) and np.array_equal(arg.cpu().numpy(), rarg)
    dx = host(ops.spp_max_bwd(arg, dev(dout), x.shape))
    assert rel(dx, _spp_max_bwd(rarg, dout, x.shape)) < TOL
    for n in range(2):
        assert abs(dx[n].sum() - dout[n].sum()) < TOL * np.abs(dout[n]).sum()
        assert np.array_equal(np.flatnonzero(dx[n]), np.unique(rarg[n]))
    # e + 1 is a channel of the same pixel, so it shares every bin with e and gets nothing; e + 3 x 256 lies in other bins of the finer levels and leads those
    assert dx[0].reshape(-1)[e] != 0 and dx[0].reshape(-1)[e + 1] == 0


# spp_avg has no earlier direct test; TOL_RED is the bound of the suite's long float32 sums.  float32 on the CPU: forward <= 7.0e-8, backward <= 3.3e-8
@pytest.mark.parametrize('C', [4, 1])
def test_spp_avg_bins_of_up_to_7040_elements(C):
    """Average pool forward and backward; C = 1 reads a channel slice of a 3-channel buffer (ldx = 3 != C)."""
    from poisson_cnn_amd import ops
    x, dout, bins = spp_inputs(C)
    bd = torch.tensor(bins, device='cuda')
    xd = dev(x)
    if C == 1:
        buf = torch.full((2, 40, 44, 3), 1e6, device='cuda')
        buf[..., 1:2] = xd
        xd = buf[..., 1:2]
        assert not xd.is_contiguous()
    assert rel(host(ops.spp_avg_fwd(xd, bd)), _spp_avg(x, bins)) < TOL_RED
    assert rel(host(ops.spp_avg_bwd(bd, dev(dout), x.shape)), _spp_avg_bwd(bins, dout, x.shape)) < TOL


# ----------------------------------------------------------------------------- 5. loss partials (64 splits x 1024 threads per sample) and backward
# hw = 1, 63, 64, 65 (most of the 64 splits are empty), 65535 (1024 per split: exactly one full trip), 67591 (1057 per split: a second trip of 33 threads)
LOSS_GRIDS = [(1, 1), (7, 9), (8, 8), (5, 13), (257, 255), (263, 257)]


def _loss_partials(p, t, G, lp):
    d = p - t
    third = (G * (t - p) ** lp).sum((1, 2)) if G is not None else 0 * d.sum((1, 2))
    return np.stack([np.abs(d).sum((1, 2)), (d * d).sum((1, 2)), third, np.abs(t).max((1, 2))], 1)


def _loss_bwd(p, t, G, cm, cs, ci, lp):
    d, c = p - t, lambda v: v[:, None, None]
    g = c(cm) * np.sign(d) + 2 * d * c(cs)
    return g + c(ci) * G * -lp * (t - p) ** (lp - 1) if G is not None else g


def loss_inputs(N, H, W):
    """Target, prediction (target - prediction = N(1, 1): mostly one sign, so the odd-power integral is no cancelling sum, and both signs occur), weights G,
    the three coefficient vectors.  max|target| sits at the LAST element of every sample, negative in sample 1."""
    rng = np.random.default_rng(H * 1000 + W)
    t = f32(rng.standard_normal((N, H, W)))
    t[:, -1, -1] = f32(np.abs(t).max() + 1.0) * np.array([1.0, -1.0, 1.0])[:N]
    p = f32(t - (rng.standard_normal((N, H, W)) + 1.0))
    return (t, p, f32(rng.uniform(0.5, 1.5, (H, W)))) + tuple(f32(rng.uniform(0.1, 1, N)) for _ in range(3))


@pytest.mark.parametrize('lp', [2, 3])
@pytest.mark.parametrize('H,W', LOSS_GRIDS)
def test_loss_partials_and_backward_from_one_element_to_a_second_trip(H, W, lp):
    from poisson_cnn_amd import ops
    t, p, G, cm, cs, ci = loss_inputs(3, H, W)
    td, pd = dev(t), dev(p)
    for Gn in (G, None):
        Gd = dev(Gn) if Gn is not None else None
        part, ref = host(ops.loss_partials(pd, td, Gd, lp_power=float(lp))), _loss_partials(p, t, Gn, lp)
        for col in range(3):
            assert rel(part[:, col], ref[:, col]) < TOL_RED, (col, rel(part[:, col], ref[:, col]))
        assert np.array_equal(part[:, 3], ref[:, 3])             # a maximum is exact
        g = ops.loss_bwd(pd, td, Gd, dev(cm), dev(cs), dev(ci), lp_power=float(lp))
        assert rel(host(g), _loss_bwd(p, t, Gn, cm, cs, ci, lp)) < TOL


# float32 on the CPU at this size: the three sums <= 1.4e-7, so TOL_RED holds
def test_loss_backward_above_the_grid_cap():
    """N hw = 2 x 1449 x 1448 = 4 196 304 > 16384 blocks x 256 threads: the grid-stride loop wraps; the whole tensor and its last 2000 elements.  The partials
    take 33 trips per split at this size."""
    from poisson_cnn_amd import ops
    t, p, G, cm, cs, ci = loss_inputs(2, 1449, 1448)
    assert t.size > 16384 * 256
    td, pd, Gd = dev(t), dev(p), dev(G)
    g = host(ops.loss_bwd(pd, td, Gd, dev(cm), dev(cs), dev(ci)))
    ref = _loss_bwd(p, t, G, cm, cs, ci, 2)
    assert rel(g, ref) < TOL and rel(g.ravel()[-2000:], ref.ravel()[-2000:]) < TOL
    for lp in (2, 3):
        part, ref = host(ops.loss_partials(pd, td, Gd, lp_power=float(lp))), _loss_partials(p, t, G, lp)
        assert all(rel(part[:, col], ref[:, col]) < TOL_RED for col in range(3)) and np.array_equal(part[:, 3], ref[:, 3])


# ----------------------------------------------------------------------------- 6. set_max_magnitude (1024 threads per sample, q += 1024)
SMM_PER = [1, 1023, 1024, 1025, 5000]


def _set_max_magnitude(x, T):
    f = T / np.abs(x).max(1)
    return x * f[:, None], f


def _set_max_magnitude_bwd(x, g, T):
    """y = x T / A, A = max|x| held by K elements: dx = g T / A - [|x| = A] sign(x) (sum g x) T / (A^2 K) - tf.reduce_max splits its gradient evenly over ties."""
    A = np.abs(x).max(1, keepdims=True)
    hit = np.abs(x) == A
    return g * T / A - hit * np.sign(x) * (g * x).sum(1, keepdims=True) * T / (A * A * hit.sum(1, keepdims=True, dtype=x.dtype))


def smm_inputs(per):
    """Sample 0: a negative maximum at the last element.  Sample 1: a two-way tie, at p and p + 2 x 1024 + 5 where the sample is long enough (another thread,
    two trips later), else at the two ends.  Sample 2: no special element."""
    rng = np.random.default_rng(per)
    x = f32(rng.standard_normal((3, per)))
    top = f32(np.abs(x).max() + 0.5)
    x[0, -1] = -top
    lo, hi = (100, 100 + 2 * 1024 + 5) if per > 2200 else (0, per - 1)
    x[1, lo], x[1, hi] = top, -top
    return x, f32(rng.standard_normal((3, per)))


@pytest.mark.parametrize('per', SMM_PER)
def test_set_max_magnitude_samples_past_one_trip(per):
    from poisson_cnn_amd import ops
    from poisson_cnn_amd.dataset import _kernels as K
    x, g = smm_inputs(per)
    T = np.array([1.0, 2.0, 0.5])
    ry, rf = _set_max_magnitude(x, T)
    xd = dev(x)
    fac = K.set_max_magnitude(xd, dev(T))                          # in place
    assert rel(host(xd), ry) < 1e-6 and np.allclose(host(fac), rf, rtol=1e-5)
    ry, rf = _set_max_magnitude(x, 0.75)
    y, fac = ops.set_max_magnitude_fwd(dev(x), 0.75)
    assert rel(host(y), ry) < 1e-6 and np.allclose(host(fac), rf, rtol=1e-5)
    dx, ref = host(ops.set_max_magnitude_bwd(dev(x), dev(g), 0.75)), _set_max_magnitude_bwd(x, g, 0.75)
    if per == 1:
        # a sample of one element is its own maximum: the gradient g T / A - g T / A is exactly 0 and the kernel leaves the rounding of its two terms,
        # so the error is measured against one of them
        assert np.linalg.norm(dx - ref) < 2e-6 * np.linalg.norm(g * 0.75 / np.abs(x))
    else:
        assert rel(dx, ref) < 2e-6                                 # (a tie that is not split is an error of 0.08 here)


# ----------------------------------------------------------------------------- 7. grid-stride wrap of the element-wise kernels
N_WRAP = GRID_CAP + 257
ADAM = tuple(float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-7))       # lr, beta_1, beta_2, epsilon as the kernel receives them
# A step is formed in float64 from the float32 weights before and after it, so it carries the rounding of the weight it was added to: half an ulp of |w| ~ 1 on a
# step of |lr| ~ 1e-3 (Adam).  Measured rel-L2 of the float32 CPU step against the float64 rule on these inputs, the largest over the two steps, the whole
# array and its last 257 elements; the bounds are 4 x the figures.
STEP_MEASURED = {'adam': 4.05e-5, 'sgd': 2.04e-6, 'momentum': 1.02e-6, 'nesterov': 8.18e-7}


def _adam_rule(g, m, v, vhat, t, lr, b1, b2, eps):
    """tf.keras Adam / AMSGrad: returns (step, m, v, vhat)."""
    m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
    if vhat is not None:
        vhat = np.maximum(vhat, v)
    lr_t = lr * float(np.sqrt(1 - b2 ** t)) / (1 - b1 ** t)
    return -lr_t * m / (np.sqrt(vhat if vhat is not None else v) + eps), m, v, vhat


def _momentum_rule(g, v, lr, mom, nesterov):
    """tf.keras SGD(momentum, nesterov): returns (step, v)."""
    v = mom * v - lr * g
    return (mom * v - lr * g if nesterov else v), v


def wrap_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return f32(rng.standard_normal(n)), [f32(rng.standard_normal(n) / (k + 1)) for k in range(2)]      # shrinking gradients: vhat > v on step 2


def _check_step(before, after, ref, bound, tail=257):
    step = after - before
    assert rel(step, ref) < bound and rel(step[-tail:], ref[-tail:]) < bound, (rel(step, ref), rel(step[-tail:], ref[-tail:]), bound)
    assert (after[-tail:] != before[-tail:]).all()


@pytest.mark.parametrize('amsgrad', [False, True])
def test_adam_steps_above_the_grid_cap(amsgrad):
    """n = 8192 x 256 + 257: the last 257 elements are reached only by the second trip of the grid-stride loop.  Two steps; each step (w after - w before, in
    float64) against the update rule, over the whole array and over that tail, and the moments."""
    from poisson_cnn_amd import ops
    w0, gs = wrap_inputs(N_WRAP, 70 + amsgrad)
    w, m, v = dev(w0), ops.zeros((N_WRAP,)), ops.zeros((N_WRAP,))
    vh = ops.zeros((N_WRAP,)) if amsgrad else None
    rm, rv, rvh = np.zeros(N_WRAP), np.zeros(N_WRAP), np.zeros(N_WRAP) if amsgrad else None
    for t, g in enumerate(gs, 1):
        before = host(w)
        ops.adam_step(w, dev(g), m, v, *ADAM, t, vhat=vh)
        ref, rm, rv, rvh = _adam_rule(g, rm, rv, rvh, t, *ADAM)
        _check_step(before, host(w), ref, max(TOL, 4 * STEP_MEASURED['adam']))
    assert rel(host(m), rm) < TOL and rel(host(v), rv) < TOL and (not amsgrad or rel(host(vh), rvh) < TOL)
    assert rel(host(m)[-257:], rm[-257:]) < TOL and rel(host(v)[-257:], rv[-257:]) < TOL


@pytest.mark.parametrize('kind', ['sgd', 'momentum', 'nesterov'])
def test_sgd_steps_above_the_grid_cap(kind):
    from poisson_cnn_amd import ops
    w0, gs = wrap_inputs(N_WRAP, 80 + len(kind))
    lr, mom, scale = (float(np.float32(c)) for c in (0.05, 0.9, 0.5))
    w, v, rv = dev(w0), ops.zeros((N_WRAP,)), np.zeros(N_WRAP)
    for g in gs:
        before = host(w)
        if kind == 'sgd':
            ops.sgd_step(w, dev(g), lr, grad_scale=scale)
            ref = -lr * scale * g
        else:
            ops.sgd_momentum_step(w, dev(g), v, lr, mom, kind == 'nesterov', grad_scale=scale)
            ref, rv = _momentum_rule(scale * g, rv, lr, mom, kind == 'nesterov')
        _check_step(before, host(w), ref, max(TOL, 4 * STEP_MEASURED[kind]))
    assert kind == 'sgd' or (rel(host(v), rv) < TOL and rel(host(v)[-257:], rv[-257:]) < TOL)


def test_axpby_above_the_grid_cap_between_two_channel_slices():
    """npix C = 8192 x 256 + 258 with x a 2-channel slice of a 4-channel buffer and y a 2-channel slice of a 3-channel one (ldx = 4, ldy = 3, C = 2)."""
    from poisson_cnn_amd import ops
    rng = np.random.default_rng(9)
    npix = GRID_CAP // 2 + 129
    bx, by = f32(rng.standard_normal((1, 1, npix, 4))), f32(rng.standard_normal((1, 1, npix, 3)))
    bxd, byd = dev(bx), dev(by)
    ops.axpby(0.5, bxd[..., 1:3], 2.0, byd[..., 0:2])
    ref = by.copy()
    ref[..., 0:2] = 0.5 * bx[..., 1:3] + 2.0 * by[..., 0:2]
    got = host(byd)
    assert rel(got, ref) < TOL and rel(got[0, 0, -129:, :2], ref[0, 0, -129:, :2]) < TOL
    assert np.array_equal(got[..., 2], by[..., 2]) and (got[0, 0, -129:, :2] != by[0, 0, -129:, :2]).all()


# ----------------------------------------------------------------------------- 8. multi-block partial sums of the scale gradients
def scale_inputs(N, C):
    """x and dy with mean 1: the sums over 90 000 pixels do not cancel, so one dropped pixel (1.1e-5 of a sum) is visible at TOL_RED."""
    rng = np.random.default_rng(300 + C)
    shape = (N, 300, 300, C)
    return f32(rng.standard_normal(shape) + 1.0), f32(rng.standard_normal(shape) + 1.0)


def _pixel_sums(a):
    """Sum over the pixels of (N, H, W, C) -> (N, C), along a contiguous axis: NumPy then adds pairwise, in float32 too."""
    return np.ascontiguousarray(np.moveaxis(a, 3, 1)).reshape(a.shape[0], a.shape[3], -1).sum(2)


# float32 on the CPU: ds <= 5.1e-8 at every C, so TOL_RED holds at hw = 90 000
@pytest.mark.parametrize('C', [1, 3, 32])
def test_channel_scale_bwd_with_many_partial_blocks_per_sample(C):
    """hw = 300 x 300: 22 (C = 1), 88 (C = 3) and the capped 256 (C = 32) partial blocks per sample, combined in a fixed order: two runs agree bit for bit."""
    from poisson_cnn_amd import ops
    x, dy = scale_inputs(2, C)
    s = f32(np.random.default_rng(C).standard_normal((2, C)))
    xd, sd, dyd = dev(x), dev(s), dev(dy)
    dx, ds = ops.channel_scale_bwd(xd, sd, dyd)
    assert rel(host(dx), dy * s[:, None, None, :]) < TOL and rel(host(ds), _pixel_sums(dy * x)) < TOL_RED
    dx2, ds2 = ops.channel_scale_bwd(xd, sd, dyd)
    assert torch.equal(ds, ds2) and torch.equal(dx, dx2)


# float32 on the CPU: dg <= 7.7e-8, so TOL_RED holds at per = 90 000
def test_sample_scale_bwd_with_64_partial_blocks_per_sample():
    from poisson_cnn_amd import ops
    x, dy = scale_inputs(3, 1)
    g = f32(np.random.default_rng(1).standard_normal(3))
    xd, gd, dyd = dev(x), dev(g), dev(dy)
    dx, dg = ops.sample_scale_bwd(xd, gd, dyd)
    assert rel(host(dx), dy * (1 + g)[:, None, None, None]) < TOL and rel(host(dg), _pixel_sums(dy * x)[:, 0]) < TOL_RED
    dx2, dg2 = ops.sample_scale_bwd(xd, gd, dyd)
    assert torch.equal(dg, dg2) and torch.equal(dx, dx2)
