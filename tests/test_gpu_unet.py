"""The UNet baseline model (poisson_cnn_amd.unet) against its fp64 torch twin (tests/unet_twin.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poisson_cnn_amd import configs
from poisson_cnn_amd.losses import loss_wrapper
from poisson_cnn_amd.train import Adam
from poisson_cnn_amd.unet import UNet
from tests import unet_twin as TW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm())


def model_and_data(cfg, N, H, W, seed=0):
    m = UNet(**cfg, seed=seed)
    rng = np.random.default_rng(seed + 10)
    ws = m.get_weights()
    # biases random too, so that every path carries signal; kernels keep the reference's initialisation
    m.set_weights([w if w.ndim > 1 else rng.uniform(-0.1, 0.1, w.shape).astype(np.float32) for w in ws])
    rhs = torch.from_numpy(rng.uniform(-1, 1, (N, 1, H, W)).astype(np.float32))
    return m, rhs


def flat_grad(m, P):
    return torch.cat([P[n].grad.reshape(-1) for n in m.weight_names])


@pytest.mark.parametrize('which', ['tiny', 'full'])
@pytest.mark.parametrize('hw', [(97, 101), (104, 104)])
def test_forward_and_gradients(which, hw):
    cfg = (configs.unet_tiny() if which == 'tiny' else configs.unet())['model']
    m, rhs = model_and_data(cfg, 2, *hw)
    pred = m(rhs)
    P = TW.params(m, requires_grad=True)
    ref = TW.forward(m, P, rhs.double())
    assert rel(pred, ref) <= 1e-5
    assert (pred >= 0).all()
    # gradient of the UNet.json loss
    full = configs.unet()
    loss = loss_wrapper(global_batch_size=2, **full['training']['loss_parameters'])
    y = torch.from_numpy(np.random.default_rng(3).uniform(0, 0.5, rhs.shape).astype(np.float32)).cuda()
    dx = torch.full((2, 2), 0.02, device='cuda')
    pred = m.call(rhs, training=False)
    _, dpred = loss.value_and_grad(y, pred, rhs.cuda(), dx)
    m.backward(dpred)
    ref.mul(dpred.double().cpu()).sum().backward()
    gm = m.store.flat_g.clone()
    gr = flat_grad(m, P)
    assert rel(gm, gr) <= 2e-4
    # autograd.Differentiable: the same kernels, bit for bit
    from poisson_cnn_amd.autograd import Differentiable
    mod = Differentiable(m)
    m.dropout_rate = 0.0
    out = mod(rhs.cuda())
    out.backward(dpred)
    m.dropout_rate = 0.5
    assert torch.equal(mod.weight.grad, gm)


def test_dropout_training_call():
    cfg = dict(configs.unet_tiny()['model'], dropout_rate=0.3)
    m, rhs = model_and_data(cfg, 2, 40, 44, seed=4)
    pred = m(rhs, training=True)
    P = TW.params(m, requires_grad=True)
    ref = TW.forward(m, P, rhs.double(), drop=(0.3, m._call_seed))
    assert rel(pred, ref) <= 1e-5
    dpred = torch.randn(pred.shape, device='cuda')
    m.backward(dpred)
    ref.mul(dpred.double().cpu()).sum().backward()
    assert rel(m.store.flat_g, flat_grad(m, P)) <= 2e-4
    assert not torch.equal(m(rhs, training=True), m(rhs, training=False))


def test_train_step_adam_and_presize():
    full = configs.unet_tiny()
    m, rhs = model_and_data(full['model'], 2, 48, 52, seed=5)
    opt = Adam(learning_rate=1e-3)
    m.compile(loss=loss_wrapper(global_batch_size=2, **full['training']['loss_parameters']), optimizer=opt)
    w0 = m.store.flat_w.clone()
    m.presize((2, 64, 64))
    assert torch.equal(m.store.flat_w, w0)
    y = torch.rand(rhs.shape) * 0.3
    dx = torch.full((2, 1), 0.02)
    # the twin's step: gradient without dropout, then Adam(1e-3) from zero moments: w - lr * g / (|g| + eps) to first order
    pred0 = m.call(rhs, training=False)
    _, dpred = m.loss_fn.value_and_grad(y.cuda(), pred0, rhs.cuda(), torch.cat([dx, dx], 1).cuda())
    P = TW.params(m, requires_grad=True)
    TW.forward(m, P, rhs.double()).mul(dpred.double().cpu()).sum().backward()
    g = flat_grad(m, P)
    logs = m.train_step(((rhs, dx), y))
    assert set(logs) == {'loss', 'mse', 'grad L2 norm', 'lr'}
    gl2 = np.sqrt(np.mean([float((P[n].grad ** 2).sum()) for n in m.weight_names]))
    assert abs(float(logs['grad L2 norm']) / gl2 - 1) < 1e-3
    step = (m.store.flat_w - w0).double().cpu()
    expect = -1e-3 * g / (g.abs() + 1e-7)
    sel = g.abs() > 1e-2 * g.abs().max()
    assert rel(step[sel], expect[sel]) <= 3e-3


def test_fit_loss_decreases():
    from poisson_cnn_amd.dataset import reverse_poisson_dataset_generator
    full = configs.unet_tiny()
    d = dict(full['dataset'], batch_size=4, batches_per_epoch=20, random_output_shape_range=[[128, 128], [128, 128]])
    ds = reverse_poisson_dataset_generator(**d)
    m = UNet(**full['model'], seed=1)
    m.compile(loss=loss_wrapper(global_batch_size=4, **full['training']['loss_parameters']), optimizer=Adam(learning_rate=1e-3))
    hist = {'l': []}

    class Rec:
        def set_model(self, model):
            pass

        def on_batch_end(self, b, logs):
            hist['l'].append(logs['loss'])

        def on_epoch_end(self, e, logs):
            pass
    m.fit(ds, epochs=1, callbacks=[Rec()], verbose=0)
    l = np.array(hist['l'])
    assert np.isfinite(l).all() and l[-5:].mean() < l[:5].mean()


def test_train_cli_one_epoch(tmp_path):
    cfg = configs.unet_tiny()
    p = tmp_path / 'unet.json'
    configs.dump_config(cfg, str(p))
    r = subprocess.run([sys.executable, '-m', 'poisson_cnn_amd.train', str(p), '--model', 'unet', '--epochs', '1', '--checkpoint_dir', str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(str(tmp_path / 'chkpt.checkpoint.npz'))
