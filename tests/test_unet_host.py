"""UNet baseline (poisson_cnn_amd.unet <- models/UNet.py): structure, initialisation, configuration plumbing and the dropout hash - no GPU."""
import numpy as np
import pytest

from poisson_cnn_amd import configs, ops
from poisson_cnn_amd.unet import UNet


def unet_param_count(depth, root, k, cin, cout, pool):
    """Re-derived from models/UNet.py: per ConvBlock two k x k convs; deconvupscale (pool, pool, F_i, F_{i+1}) + bias; a 1x1 head."""
    F = [2 ** i * root for i in range(depth)]
    n, c = 0, cin
    for i in range(depth - 1):
        n += k * k * c * F[i] + F[i] + k * k * F[i] * F[i] + F[i]
        c = F[i]
    n += k * k * c * F[-1] + F[-1] + k * k * F[-1] * F[-1] + F[-1]
    for i in range(depth - 2, -1, -1):
        n += pool * pool * F[i] * F[i + 1] + F[i]
        n += k * k * 2 * F[i] * F[i] + F[i] + k * k * F[i] * F[i] + F[i]
    return n + F[0] * cout + cout


def test_param_count_unet_json():
    m = UNet(**configs.unet()['model'], device='cpu')
    assert m.count_params() == 7696193 == unet_param_count(4, 64, 3, 1, 1, 2)
    assert UNet(**configs.unet_tiny()['model'], device='cpu').count_params() == unet_param_count(3, 8, 3, 1, 1, 2)


def test_weight_names_and_shapes_follow_keras_order():
    m = UNet(**configs.unet()['model'], device='cpu')
    names = m.weight_names
    conv = ['conv_block%s/conv2d%s' % ('_%d' % (i // 2) if i // 2 else '', '_%d' % i if i else '') for i in range(14)]
    blocks = [conv[0:2], conv[2:4], conv[4:6], conv[6:8]]
    expect = []
    for b in blocks:
        for c in b:
            expect += [c + '/kernel', c + '/bias']
    for j in range(3):
        d = 'deconvupscale' + ('_%d' % j if j else '')
        expect += [d + '/kernel', d + '/bias']
        for c in conv[8 + 2 * j: 10 + 2 * j]:
            expect += [c.replace('conv_block_%d' % (int(c.split('_')[-1]) // 2), 'conv_block_%d' % (4 + j)) + '/kernel', None]
    # names of the expanding blocks: conv_block_4.. hold conv2d_8..13
    exp_names = [n for n in expect if n is not None]
    assert names[:16] == exp_names[:16]
    assert names[-2:] == ['conv2d_14/kernel', 'conv2d_14/bias']
    shapes = dict(zip(names, [w.shape for w in m.get_weights()]))
    F = [64, 128, 256, 512]
    assert shapes['conv_block/conv2d/kernel'] == (3, 3, 1, 64)
    assert shapes['conv_block_3/conv2d_7/kernel'] == (3, 3, 512, 512)
    assert shapes['deconvupscale/kernel'] == (2, 2, 256, 512) and shapes['deconvupscale/bias'] == (256,)
    assert shapes['conv_block_4/conv2d_8/kernel'] == (3, 3, 512, 256)
    assert shapes['deconvupscale_2/kernel'] == (2, 2, 64, 128)
    assert shapes['conv_block_6/conv2d_12/kernel'] == (3, 3, 128, 64)
    assert shapes['conv2d_14/kernel'] == (1, 1, 64, 1)
    assert all(shapes[n] == (F[0] if '14' not in n else 1,) for n in names if n.endswith('bias') and ('conv2d_13' in n or 'conv2d_14' in n))


def test_truncated_normal_init():
    m = UNet(**configs.unet()['model'], device='cpu', seed=3)
    for name, std in m._trunc.items():
        v = m.store.w[name].numpy().ravel()
        assert np.abs(v).max() <= 2 * std * (1 + 1e-6), name
        if v.size >= 4096:
            # a normal truncated at 2 sigma has standard deviation 0.8796 sigma
            assert abs(v.std() / 0.879626 / std - 1) < 0.03, (name, v.std(), std)
    assert m._trunc['conv_block_3/conv2d_7/kernel'] == pytest.approx(np.sqrt(2 / (9 * 512)))
    assert m._trunc['conv2d_14/kernel'] == pytest.approx(np.sqrt(2 / (9 * 64)))          # _get_kernel_initializer(filters_root, kernel_size)
    for n in m.weight_names:
        if n.startswith('conv') and n.endswith('bias'):
            assert not m.store.w[n].numpy().any()


def test_padding_valid_raises():
    cfg = dict(configs.unet()['model'], padding='valid')
    with pytest.raises(NotImplementedError, match="padding='same'"):
        UNet(**cfg, device='cpu')


def test_dropout_hash_rate_and_determinism():
    for rate in (0.5, 0.2):
        m = ops.dropout_keep_mask((1000, 1000), rate, seed=7, layer=3)
        assert abs(1 - m.mean() - rate) < 0.01 * rate + 1e-3
        assert np.array_equal(m, ops.dropout_keep_mask((1000, 1000), rate, seed=7, layer=3))
        assert not np.array_equal(m, ops.dropout_keep_mask((1000, 1000), rate, seed=8, layer=3))
        assert not np.array_equal(m, ops.dropout_keep_mask((1000, 1000), rate, seed=7, layer=4))
    assert ops.dropout_keep_mask((100,), 0.0, 1, 1).all()


def test_train_unet_argument_parsing(monkeypatch, tmp_path):
    import poisson_cnn_amd.train as tr
    import poisson_cnn_amd.unet as U
    seen = {}

    class Stop(Exception):
        pass

    def fake_unet(**kw):
        seen['model'] = kw
        raise Stop
    monkeypatch.setattr(U, 'UNet', fake_unet)
    import poisson_cnn_amd.dataset as D

    def fake_gen(**kw):
        seen['dataset'] = kw
        return None
    monkeypatch.setattr(D, 'reverse_poisson_dataset_generator', fake_gen)
    cfg = configs.unet()
    p = tmp_path / 'unet.json'
    configs.dump_config(cfg, str(p))
    with pytest.raises(Stop):
        tr.main([str(p), '--model', 'unet', '--epochs', '1'])
    assert seen['model'] == cfg['model']
    assert seen['dataset']['random_output_shape_range'] == [[192, 384], [192, 384]] and seen['dataset']['batch_size'] == 50
    with pytest.raises(SystemExit):
        tr.main([str(p), '--model', 'nope'])
