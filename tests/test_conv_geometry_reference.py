"""CPU: the geometry-general fp64 reference of tests/conv_geometry.py, pinned independently of the oracle it is built from - against
numpy.pad + torch.nn.functional.conv2d in float64, for the three pad modes, rectangular filters, unequal offsets in the two axes, VALID
convolutions and pads at the tf.pad limit, to 1e-12 - and its helpers (regions, gamma)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_geometry as G

NP_MODE = {'CONSTANT': 'constant', 'SYMMETRIC': 'symmetric', 'REFLECT': 'reflect'}

# kh, kw, pad_top, pad_left, H, W, Ho, Wo
GEOMS = [(3, 7, 1, 3, 12, 14, 12, 14), (7, 3, 3, 1, 12, 14, 12, 14), (15, 9, 7, 4, 20, 17, 20, 17), (9, 15, 4, 7, 17, 20, 17, 20), (13, 5, 6, 2, 16, 11, 16, 11),
         (4, 13, 2, 6, 15, 16, 15, 16), (13, 4, 6, 2, 16, 15, 16, 15), (2, 15, 1, 7, 9, 18, 9, 18), (6, 11, 3, 5, 13, 14, 13, 14),
         (7, 7, 1, 5, 12, 13, 10, 14), (5, 9, 4, 0, 11, 15, 12, 9),             # unequal offsets, Ho / Wo adjusted
         (5, 9, 0, 0, 11, 15, 7, 7), (11, 3, 0, 0, 14, 9, 4, 7),                # VALID
         (14, 15, 13, 14, 15, 16, 28, 30)]                                       # the padded domain (pad = k - 1 on both sides)


def independent(x, w, b, pt, pl, out_hw, mode, value):
    kh, kw = w.shape[:2]
    pb = out_hw[0] - 1 - pt + kh - 1 - (x.shape[2] - 1)
    pr = out_hw[1] - 1 - pl + kw - 1 - (x.shape[3] - 1)
    kwargs = {'constant_values': value} if mode == 'CONSTANT' else {}
    xp = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)), mode=NP_MODE[mode], **kwargs)
    return F.conv2d(torch.tensor(xp), torch.tensor(w).permute(3, 2, 0, 1).contiguous(), torch.tensor(b))


@pytest.mark.parametrize('mode', ['CONSTANT', 'SYMMETRIC', 'REFLECT'])
@pytest.mark.parametrize('kh,kw,pt,pl,H,W,Ho,Wo', GEOMS)
def test_reference_and_twin_match_numpy_pad_and_torch_conv2d(kh, kw, pt, pl, H, W, Ho, Wo, mode):
    rng = np.random.default_rng(kh * 100 + kw)
    N, Cin, Cout = 2, 3, 4
    x = rng.standard_normal((N, Cin, H, W))
    w = rng.standard_normal((kh, kw, Cin, Cout)) / np.sqrt(kh * kw * Cin)
    b = rng.standard_normal(Cout)
    dz = rng.standard_normal((N, Cout, Ho, Wo))
    assert G.pads_of(H, W, kh, kw, pt, pl, (Ho, Wo))[0][0] == pt and G.pads_of(H, W, kh, kw, pt, pl, (Ho, Wo))[1][0] == pl
    xt, wt, bt = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    # the independent construction, differentiable through an index map built by numpy.pad itself
    (pt_, pb_), (pl_, pr_) = G.pads_of(H, W, kh, kw, pt, pl, (Ho, Wo))
    kwargs = {'constant_values': -1} if mode == 'CONSTANT' else {}
    iy = np.pad(np.arange(H), (pt_, pb_), mode=NP_MODE[mode], **kwargs)
    ix = np.pad(np.arange(W), (pl_, pr_), mode=NP_MODE[mode], **kwargs)
    xp = xt[:, :, np.maximum(iy, 0)][:, :, :, np.maximum(ix, 0)]
    inside = torch.tensor((iy >= 0)[:, None] & (ix >= 0)[None, :])
    xp = torch.where(inside, xp, torch.tensor(0.3, dtype=torch.float64))
    want = F.conv2d(xp, wt.permute(3, 2, 0, 1), bt)
    assert float((want.detach() - independent(x, w, b, pt, pl, (Ho, Wo), mode, 0.3)).abs().max()) == 0.0
    (torch.tanh(want) * torch.tensor(dz)).sum().backward()
    scale = float(want.detach().abs().max())
    got = G.ref_conv(x, w, b, pt, pl, (Ho, Wo), mode, 0.3, 'linear')
    assert got.shape == (N, Cout, Ho, Wo)
    assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * scale
    twin = G.twin_conv(torch.tensor(x), torch.tensor(w), torch.tensor(b), pt, pl, (Ho, Wo), mode, 0.3, 'tanh')
    assert float((twin - torch.tanh(want.detach())).abs().max()) <= 1e-12
    assert np.abs(G.ref_conv(x, w, b, pt, pl, (Ho, Wo), mode, 0.3, 'tanh') - twin.numpy()).max() <= 1e-12
    dx, dw, db = G.gradients(x, w, b, dz, pt, pl, mode, 0.3, 'tanh')
    for g, r in ((dx, xt.grad), (dw, wt.grad), (db, bt.grad)):
        assert np.abs(g - r.numpy()).max() <= 1e-12 * max(1.0, float(r.abs().max()))


def test_offsets_are_literal():
    """One hot pixel, one hot tap: output (oy, ox) reads input row oy - pad_top + ty and column ox - pad_left + tx - checked by position, so
    an exchange of the two axes in the reference itself cannot hide."""
    kh, kw, pt, pl, H, W = 5, 9, 4, 0, 11, 15
    Ho, Wo = 12, 9
    x = np.zeros((1, 1, H, W)); x[0, 0, 6, 10] = 1.0
    w = np.zeros((kh, kw, 1, 1)); w[1, 7, 0, 0] = 1.0
    y = G.ref_conv(x, w, None, pt, pl, (Ho, Wo))
    oy, ox = 6 + pt - 1, 10 + pl - 7
    assert y[0, 0, oy, ox] == 1.0 and y.sum() == 1.0
    dx, dw, db = G.gradients(x, w, None, y, pt, pl)
    assert db is None and dw[1, 7, 0, 0] == 1.0 and dw.sum() == 1.0 and dx[0, 0, 6, 10] == 1.0 and dx.sum() == 1.0


def test_pad_at_and_beyond_the_tf_pad_limit():
    """SYMMETRIC accepts pad == size, REFLECT pad == size - 1; one step beyond raises, in the numpy reference and in the twin, per axis."""
    rng = np.random.default_rng(0)
    w = rng.standard_normal((15, 15, 2, 3))
    for axis in (0, 1):
        for mode, ok, bad in (('SYMMETRIC', 7, 6), ('REFLECT', 8, 7)):
            shape = lambda n: (1, 2, n, 20) if axis == 0 else (1, 2, 20, n)
            x = rng.standard_normal(shape(ok))
            y = G.ref_conv(x, w, None, 7, 7, x.shape[2:], mode)
            assert np.abs(y - G.twin_conv(torch.tensor(x), torch.tensor(w), None, 7, 7, x.shape[2:], mode).numpy()).max() <= 1e-12
            x = rng.standard_normal(shape(bad))
            with pytest.raises(ValueError, match='exceeds'):
                G.ref_conv(x, w, None, 7, 7, x.shape[2:], mode)
            with pytest.raises(ValueError, match='exceeds'):
                G.twin_conv(torch.tensor(x), torch.tensor(w), None, 7, 7, x.shape[2:], mode)
    with pytest.raises(ValueError, match='negative'):
        G.ref_conv(rng.standard_normal((1, 2, 20, 20)), w, None, 7, 7, (10, 20))


def test_regions_and_gamma():
    y = np.arange(2 * 3 * 9 * 11, dtype=np.float64).reshape(2, 3, 9, 11) + 1.0
    reg = dict(G.regions(y, 3, 4))
    assert list(reg) == ['whole', 'border', 'channel 0', 'channel 1', 'channel 2', 'sample 0', 'sample 1']
    band = reg['border']
    assert np.all(band[:, :, 2:7, 3:8] == 0) and np.array_equal(band[:, :, :2], y[:, :, :2]) and np.array_equal(band[:, :, :, 8:], y[:, :, :, 8:])
    assert np.count_nonzero(band) == 2 * 3 * (9 * 11 - 5 * 5)
    assert np.array_equal(reg['channel 1'], y[:, 1]) and np.array_equal(reg['sample 1'], y[1])
    assert np.array_equal(dict(G.regions(y, 7, 3))['border'], y)            # a band as deep as half the image is the whole image
    # a defect in one channel of 32 is diluted by sqrt(32) in the whole-tensor norm and not at all in that channel's
    z = np.ones((2, 32, 5, 6)); bad = z.copy(); bad[:, 9] *= 1 + 8e-6
    assert G.rel(bad, z) < 2e-6 < 7.9e-6 < G.worst_region(bad, z, 3, 3)[1] and G.worst_region(bad, z, 3, 3)[0] == 'channel 9'
    assert G.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and G.gamma(15 * 9 * 32 + 1) == pytest.approx(4321 * 2.0 ** -24, rel=1e-3)
    # the bound holds for an fp32 evaluation in a deliberately bad order
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(4321).astype(np.float32), rng.standard_normal(4321).astype(np.float32)
    s = np.float32(0)
    for p in np.sort(a * b):
        s = np.float32(s + p)
    exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
    assert abs(float(s) - exact) <= G.gamma(4321) * float(np.dot(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64)))
