"""Homogeneous_Poisson_NN_Legacy(density_input=True), losses.variable_density_loss_wrapper and `train --dataset_type variable_density`: the tiny
model of tests/test_gpu_model.py on 24 x 28 grids against an fp64 twin put together in tests/varcoef_train_twin.py from the public pieces of
oracle/hpnn.py.  Bounds are the project's tiny-config ones: forward rel-L2 <= 1e-5, flat gradient <= 2e-4."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import hpnn as ohpnn, np_ops, torch_twin
from poisson_cnn_amd import configs
from tests import varcoef_train_twin as T

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_GRAD = 1e-5, 2e-4
N, H, W = 2, 24, 28


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) / np.linalg.norm(np.asarray(b, dtype=np.float64).ravel())


def model_cfg(iterations, **kw):
    return dict(configs.hpnn_tiny()['model'], postsmoother_iterations=iterations, **kw)


def loss_params(pi_weight, normalize=False):
    lossp = dict(configs.hpnn_tiny()['training']['loss_parameters'])
    lossp.update(physics_informed_loss_weight=pi_weight, mse_loss_weight=0.2,
                 physics_informed_loss_config={'stencil_sizes': [3, 3], 'orders': 2, 'normalize': normalize})
    return lossp


@functools.lru_cache(maxsize=None)
def batch():
    """fp32-rounded host arrays: stack (N,2,H,W) = [rhs, rho], dx (N,1), a target."""
    rng = np.random.default_rng(31)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    rhs = rng.uniform(-1, 1, (N, 1, H, W))
    rhs /= np.abs(rhs).max(axis=(1, 2, 3), keepdims=True)
    rho = rng.uniform(1.0, 10.0, (N, 1, H, W))
    return f32(np.concatenate([rhs, rho], 1)), f32(rng.uniform(5e-3, 5e-2, (N, 1))), f32(rng.standard_normal((N, 1, H, W)) * 0.1)


def build(cfg, seed=21):
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    model = Homogeneous_Poisson_NN_Legacy(**cfg)
    p = T.density_params(cfg, seed)
    model.set_weights(p)
    return model, p


def test_zero_rho_slice_is_the_one_channel_model():
    """The rho slice of the first filter zeroed, everything else copied: the forward of the one-channel model (other routes may run: 1e-5)."""
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    stack, dx, _ = batch()
    cfg = model_cfg(0)
    base = Homogeneous_Poisson_NN_Legacy(**cfg)
    p = ohpnn.init_params(cfg, seed=5, gain=1.6, randomize_all=True)
    base.set_weights(p)
    wide = Homogeneous_Poisson_NN_Legacy(**dict(cfg, density_input=True))
    k = p['pre/conv0/kernel']
    q = dict(p)
    q['pre/conv0/kernel'] = np.concatenate([k[:, :, :1], np.zeros_like(k[:, :, :1]), k[:, :, 1:]], axis=2)
    wide.set_weights(q)
    y0 = base([stack[:, :1], dx]).cpu().numpy()
    y1 = wide([stack, dx]).cpu().numpy()
    err = rel(y1, y0)
    print('zero rho slice vs one-channel model: rel-L2 %.3g' % err)
    assert np.abs(y0).max() > 0 and err <= TOL_FWD


@pytest.mark.parametrize('normalize', [False, True])
def test_forward_and_gradient_against_the_fp64_twin(normalize):
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import SGD
    stack, dx, target = batch()
    cfg = model_cfg(3, density_input=True)
    model, p = build(cfg)
    ref = T.model_forward(np_ops, cfg, p, stack, dx)
    # the residual is of order 1 / dx^2: the weight is set from the twin so that the physics-informed term equals the supervised ones
    unit = loss_params(1.0, normalize)
    supervised = float(T.density_loss(dict(unit, physics_informed_loss_weight=0.0), 4, target, torch.tensor(ref), stack, dx))
    lossp = loss_params(float(np.float32(supervised / (float(T.density_loss(unit, 4, target, torch.tensor(ref), stack, dx)) - supervised))), normalize)
    y = model([stack, dx]).cpu().numpy()
    err = rel(y, ref)
    print('forward vs fp64 twin: rel-L2 %.3g' % err)
    assert y.shape == ref.shape and err <= TOL_FWD
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=not k.endswith(('moving_mean', 'moving_variance'))) for k, v in p.items()}
    pred = T.model_forward(torch_twin, cfg, pt, torch.tensor(stack), torch.tensor(dx))
    loss = T.density_loss(lossp, 4, target, pred, stack, dx)
    loss.backward()
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=4, **lossp), optimizer=SGD(learning_rate=0.0))
    logs = model.train_step(((stack, dx), target))
    names = model.store.trainable_names()
    flat = np.concatenate([model.store.g[n].cpu().numpy().ravel() for n in names])
    flat_ref = np.concatenate([pt[n].grad.numpy().ravel() for n in names])
    gerr = rel(flat, flat_ref)
    print('loss %.6g vs %.6g, flat gradient rel-L2 %.3g' % (float(logs['loss']), float(loss.detach()), gerr))
    assert abs(float(logs['loss']) - float(loss.detach())) <= 2e-5 * abs(float(loss.detach()))
    assert gerr <= TOL_GRAD
    assert abs(float(loss.detach()) - 2.0 * supervised) <= 1e-3 * supervised                 # both halves of the loss are in this gradient


def test_adam_lowers_the_loss_on_a_generator_batch():
    from poisson_cnn_amd import dataset as D
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    gen = D.variable_density_dataset_generator(batch_size=2, output_shape=(H, W), seed=7)
    (stack, dx), soln = gen[0]
    model = build(model_cfg(2, density_input=True))[0]
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=2, **loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3))
    losses = [float(model.train_step(((stack, dx), soln))['loss']) for _ in range(10)]
    print('ten Adam steps: loss %.6g -> %.6g' % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_refusals():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    stack, dx, target = batch()
    for bc in ('neumann', {'left': 'neumann'}, {'left': 'dirichlet'}):
        with pytest.raises(NotImplementedError, match='density_input'):
            Homogeneous_Poisson_NN_Legacy(**model_cfg(0, density_input=True, bc_type=bc))
    model = build(model_cfg(0, density_input=True))[0]
    with pytest.raises(ValueError, match=r'\(N,2,H,W\)'):
        model([stack[:, :1], dx])
    assert torch.equal(model([stack, np.concatenate([dx, dx], 1)]), model([stack, dx]))         # equal columns are one spacing
    with pytest.raises(NotImplementedError, match='anisotropic'):
        model([stack, np.concatenate([dx, 2 * dx], 1)])
    from poisson_cnn_amd.train import SGD
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **loss_params(1e-9)), optimizer=SGD(learning_rate=0.0))
    with pytest.raises(NotImplementedError, match='anisotropic'):
        model.train_step(((stack, np.concatenate([dx, 2 * dx], 1)), target))
    from poisson_cnn_amd.models import Dirichlet_BC_NN_Legacy_2, Poisson_CNN_Legacy
    with pytest.raises(NotImplementedError, match='density_input'):
        Poisson_CNN_Legacy(model, Dirichlet_BC_NN_Legacy_2(**configs.dbcnn_tiny()['model']))
    lossp = loss_params(1e-9)
    for key, bad in (('stencil_sizes', [5, 5]), ('stencil_sizes', 5), ('orders', 4), ('orders', [2, 4])):
        with pytest.raises(NotImplementedError, match=key):
            variable_density_loss_wrapper(**dict(lossp, physics_informed_loss_config=dict(lossp['physics_informed_loss_config'], **{key: bad})))
    L = variable_density_loss_wrapper(**lossp)
    st, tg = torch.tensor(stack, device='cuda', dtype=torch.float32), torch.tensor(target, device='cuda', dtype=torch.float32)
    d = torch.tensor(dx, device='cuda', dtype=torch.float32)
    assert np.isfinite(float(L(tg, tg * 0.5, st, torch.cat([d, d], 1))))                     # equal columns are one spacing
    with pytest.raises(NotImplementedError, match='anisotropic'):
        L(tg, tg * 0.5, st, torch.cat([d, 2 * d], 1))
    with pytest.raises(ValueError, match=r'\(N,2,H,W\)'):
        L(tg, tg * 0.5, st[:, :1], d)


def test_checkpoints_round_trip(tmp_path):
    stack, dx, _ = batch()
    cfg = model_cfg(2, density_input=True)
    a = build(cfg)[0]
    for fmt, name in ((None, 'w'), ('tf', 'tfw')):
        a.save_weights(str(tmp_path / name), **({'save_format': fmt} if fmt else {}))
        b = build(cfg, seed=99)[0]
        b.load_weights(str(tmp_path / name))
        assert torch.equal(a.store.flat_w, b.store.flat_w), fmt
        assert torch.equal(a([stack, dx]), b([stack, dx])), fmt
    assert tuple(a.store.w['pre/conv0/kernel'].shape)[-2] == 4


def test_evaluate_reports_errors_and_leaves_the_residual_columns_zero():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    stack, dx, target = batch()
    model = build(model_cfg(2, density_input=True))[0]
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3))
    res = model.evaluate([stack, dx], target, batch_size=N, return_dict=True, per_sample=True)
    y = model([stack, dx]).cpu().numpy()
    assert abs(res['mse'] - np.mean((y - target) ** 2)) <= 1e-5 * np.mean((y - target) ** 2)
    assert res['stats'].shape == (N, 8) and (res['stats'][:, 5:] == 0).all() and (res['stats'][:, :5] > 0).all()
    assert np.isfinite(res['loss'])


def _train_config():
    cfg = configs.hpnn_tiny()
    cfg['model'].update(density_input=True, postsmoother_iterations=2)
    cfg['dataset'] = {'batch_size': 2, 'batches_per_epoch': 2, 'output_shape': [H, W]}
    cfg['training']['n_epochs'] = 1
    cfg['training']['loss_parameters'] = loss_params(1e-9)
    return cfg


def test_train_main_runs_two_steps_and_writes_a_checkpoint(tmp_path, monkeypatch):
    from poisson_cnn_amd import dataset as D, losses, models as M, train
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(_train_config()))
    seen = {}
    orig_fit = M.Homogeneous_Poisson_NN_Legacy.fit

    def fit(self, dataset, *a, **kw):
        seen['model'], seen['dataset'] = self, dataset
        seen['history'] = orig_fit(self, dataset, *a, **kw)
        return seen['history']
    monkeypatch.setattr(M.Homogeneous_Poisson_NN_Legacy, 'fit', fit)
    train.main([str(path), '--dataset_type', 'variable_density', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    assert seen['model'].density_input and isinstance(seen['model'].loss_fn, losses.variable_density_loss_wrapper)
    assert isinstance(seen['dataset'], D.variable_density_dataset_generator) and seen['model'].optimizer.iterations == 2
    assert all(np.isfinite(v) for v in seen['history']['loss']) and len(seen['history']['loss']) == 1
    assert any(f.startswith('chkpt') for f in os.listdir(tmp_path))


def test_train_main_refuses_a_mismatch_of_model_and_dataset(tmp_path):
    from poisson_cnn_amd import train
    cfg = _train_config()
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match='--dataset_type variable_density'):
        train.main([str(path), '--dataset_type', 'analytical', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    cfg['dataset']['boundaries'] = 'random'
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="boundaries 'zero'"):
        train.main([str(path), '--dataset_type', 'variable_density', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])
    cfg['dataset'].pop('boundaries')
    cfg['model'].pop('density_input')
    path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match='density_input'):
        train.main([str(path), '--dataset_type', 'variable_density', '--checkpoint_dir', str(tmp_path), '--epochs', '1'])


def test_the_public_jacobi_layer_is_the_kernels():
    from poisson_cnn_amd import keras_layers as KL, ops
    stack, dx, target = batch()
    dev = lambda a: torch.tensor(a, device='cuda', dtype=torch.float32).contiguous()
    rhs, rho, u, g = dev(stack[:, :1]), dev(stack[:, 1:]), dev(target), dev(target[::-1].copy())
    n = ops.varcoef_jacobi_k_max() + 1
    lay = KL.VariableDensityJacobiLayer(n_iterations=n)
    y = lay([u, rhs, rho, dx], training=True)
    d = dev(dx).reshape(-1)
    assert y.shape == u.shape and torch.equal(y, ops.varcoef_jacobi(u, rho, rhs, d, n))
    assert torch.equal(lay.backward(g), ops.varcoef_jacobi_bwd(g, rho, d, n))
    assert torch.equal(lay([u, rhs, rho, np.concatenate([dx, dx], 1)]), y)                        # equal columns are one spacing
    with pytest.raises(NotImplementedError, match='anisotropic'):
        lay([u, rhs, rho, np.concatenate([dx, 2 * dx], 1)])
    with pytest.raises(ValueError, match='one channel'):
        lay([u, dev(stack), rho, dx])
    with pytest.raises(NotImplementedError, match='2-D'):
        KL.VariableDensityJacobiLayer(ndims=3)
    last = KL.VariableDensityJacobiLayer(n_iterations=2, data_format='channels_last')
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(last([cl(u), cl(rhs), cl(rho), dx]), cl(ops.varcoef_jacobi(u, rho, rhs, d, 2)))
    assert torch.equal(KL.VariableDensityJacobiLayer(n_iterations=0)([u, rhs, rho, dx]), u)


def test_presize_runs_a_two_channel_batch_and_leaves_the_model_as_it_was():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    stack, dx, _ = batch()
    model = build(model_cfg(2, density_input=True))[0]
    (dummy, ddx), dtarget = model._dummy_batch((N, H, W))
    assert tuple(dummy.shape) == (N, 2, H, W) and tuple(dtarget.shape) == (N, 1, H, W)
    assert float(dummy[:, 1].min()) >= 1.0 and float(dummy[:, 1].max()) <= 2.0 and float(dummy[:, 0].min()) < 0.0
    before, y0 = model.store.flat_w.clone(), model([stack, dx])
    model.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3), max_input_shape=(N, H + 8, W + 4))
    assert torch.equal(model.store.flat_w, before) and float(model.store.flat_g.abs().max()) == 0.0 and model.optimizer.iterations == 0
    assert torch.equal(model([stack, dx]), y0)


def test_first_layer_of_the_shipped_config_with_four_input_channels():
    """The shipped model's first convolution (15 taps, SYMMETRIC padding, leaky_relu, 4 filters) with Cin = 4 = [rhs, rho, two position channels] at a
    shipped grid size: forward, weight gradient and data gradient against fp64 autograd, with the per-op bounds of tests/test_gpu_ops.py (2e-6; 5e-6
    for the filter gradient, a long fp32 reduction)."""
    from poisson_cnn_amd import ops
    k, Ci, Co, n, h, w = 15, 4, 4, 2, 192, 200
    rng = np.random.default_rng(15)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    x, wt_, b = f32(rng.standard_normal((n, Ci, h, w))), f32(rng.standard_normal((k, k, Ci, Co)) / np.sqrt(k * k * Ci)), f32(rng.uniform(-0.1, 0.1, Co))
    dz = f32(rng.standard_normal((n, Co, h, w)))
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(wt_, requires_grad=True)
    y = torch_twin.padded_conv2d(xt, wt, torch.tensor(b), 'SYMMETRIC', 0.0, 'leaky_relu')
    lin = torch_twin.padded_conv2d(xt, wt, None, 'SYMMETRIC', 0.0, 'linear')
    (lin * torch.tensor(dz)).sum().backward()
    nhwc = lambda a: torch.tensor(np.ascontiguousarray(a.transpose(0, 2, 3, 1)), dtype=torch.float32, device='cuda')
    xd, dzd, wd = nhwc(x), nhwc(dz), torch.tensor(wt_, dtype=torch.float32, device='cuda')
    p = k // 2
    yd = ops.conv2d_fwd(xd, wd, torch.tensor(b, dtype=torch.float32, device='cuda'), pad_top=p, pad_left=p, pad_mode='SYMMETRIC', act='leaky_relu')
    dw = ops.conv2d_wgrad(xd, dzd, wt_.shape, pad_top=p, pad_left=p, pad_mode='SYMMETRIC')
    gp = ops.conv2d_fwd(dzd, ops.flip_transpose_weights(wd), None, pad_top=k - 1, pad_left=k - 1, out_hw=(h + k - 1, w + k - 1))
    dxd = ops.pad_fold_bwd(gp, (h, w), ((p, k - 1 - p), (p, k - 1 - p)), 'SYMMETRIC')
    nchw = lambda t: t.cpu().numpy().transpose(0, 3, 1, 2)
    errs = rel(nchw(yd), y.detach().numpy()), rel(dw.cpu().numpy(), wt.grad.numpy()), rel(nchw(dxd), xt.grad.numpy())
    print('15-tap 4 -> 4 at %d x %d x %d: forward %.3g, filter gradient %.3g, data gradient %.3g' % ((n, h, w) + errs))
    assert errs[0] < 2e-6 and errs[1] < 5e-6 and errs[2] < 2e-6
