"""The recurrence kernels (csrc/rnn.hip through ops.rnn_fwd / rnn_bwd) and Dirichlet_BC_RNN against the fp64 twin (tests/rnn_twin.py).

Bounds are the project's own (tests/test_gpu_conv.py, tests/test_gpu_unet.py): one layer rel-L2 <= 2e-6 forward and data gradient, <= 5e-6 weight
and bias gradients; whole model <= 1e-5 forward, <= 2e-4 flat gradient.  Every parity test prints what it measured before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poisson_cnn_amd import configs, ops
from poisson_cnn_amd.losses import loss_wrapper
from poisson_cnn_amd.rnn import Dirichlet_BC_RNN, keras_initializer
from poisson_cnn_amd.train import Adam
from tests import rnn_twin as TW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, DATA, WEIGHT = 2e-6, 2e-6, 5e-6          # one layer
MODEL_FWD, MODEL_GRAD = 1e-5, 2e-4            # whole model


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    nb = float(b.norm())
    return float((a - b).norm()) / (nb if nb > 0.0 else 1.0)       # an exactly zero reference (dU at T = 1: h_0 = 0) is compared absolutely


# ----------------------------------------------------------------------------------------------------------------- one layer
def layer_data(cell, N, T, cin, u, seed, use_bias=True):
    """Inputs of the kind the model sees: a scaled random walk, Keras initialisers, biases of scale 0.1."""
    G = ops.RNN_GATES[cell]
    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.standard_normal((N, T, cin)), 1) * 0.1).astype(np.float32)
    W = keras_initializer('glorot_uniform', (cin, G * u), rng)
    U = keras_initializer('orthogonal', (u, G * u), rng)
    b = (rng.standard_normal((G * u,) if cell == 'lstm' else (2, G * u)) * 0.1).astype(np.float32) if use_bias else None
    gy = rng.standard_normal((N, T, u)).astype(np.float32)
    return [None if v is None else torch.from_numpy(v) for v in (x, W, U, b, gy)]


def gpu_layer(cell, x, W, U, b, gy, act='tanh', rec='sigmoid', go_backwards=False, sliced=False):
    """One recurrent layer from the ops wrappers alone: projection, recurrence, and every gradient.  sliced: the projected gates and the incoming
    gradient are channel slices of wider buffers, the outputs strided views."""
    N, T, cin = x.shape
    u, Gu = U.shape
    x, W, U, gy = x.cuda(), W.cuda(), U.cuda(), gy.cuda()
    b = b.cuda() if b is not None else None
    bx = None if b is None else (b if cell == 'lstm' else b[0].contiguous())
    bh = None if (b is None or cell == 'lstm') else b[1].contiguous()
    wide = lambda C: torch.full((N, T, C + 7), float('nan'), device='cuda')[:, :, 3:3 + C] if sliced else ops.empty((N, T, C), 'cuda')   # noqa: E731
    zx = wide(Gu)
    ops.wide_conv2d_fwd(x.view(N, T, 1, cin), W.view(1, 1, cin, Gu), bx, out=zx.view(N, T, 1, Gu))
    h, saved = ops.rnn_fwd(zx, U, bh, cell=cell, act=act, rec_act=rec, reverse=go_backwards, h=wide(u))
    dh = wide(u)
    dh.copy_(gy)
    dzx, dzh = ops.rnn_bwd(U, saved, h, dh, cell=cell, act=act, rec_act=rec, reverse=go_backwards)
    hprev = torch.cat([torch.zeros(N, 1, u, device='cuda'), h[:, :-1]], 1).contiguous()
    dbx = torch.zeros(Gu, device='cuda')
    dbh = torch.zeros(Gu, device='cuda')
    dW = ops.wide_conv2d_wgrad(x.view(N, T, 1, cin), dzx.view(N, T, 1, Gu), (1, 1, cin, Gu), dbias=dbx).view(cin, Gu)
    dU = ops.wide_conv2d_wgrad(hprev.view(N, T, 1, u), dzh.view(N, T, 1, Gu), (1, 1, u, Gu), dbias=dbh).view(u, Gu)
    dx = ops.wide_conv2d_dgrad(dzx.view(N, T, 1, Gu), ops.flip_transpose_weights(W.view(1, 1, cin, Gu))).view(N, T, cin)
    db = None if b is None else (dbx if cell == 'lstm' else torch.stack([dbx, dbh]))
    return h, dx, dW, dU, db


def twin_layer(cell, x, W, U, b, gy, wrong=None, **kw):
    leaves = [t.double().clone().requires_grad_(True) for t in (x, W, U)] + ([b.double().clone().requires_grad_(True)] if b is not None else [])
    y = TW.layer(cell, leaves[0], leaves[1], leaves[2], leaves[3] if b is not None else None, wrong=wrong, **kw)
    grads = torch.autograd.grad((y * gy.double()).sum(), leaves)
    return [y.detach()] + list(grads) + ([None] if b is None else [])


def layer_errors(got, ref):
    names = ('h', 'dx', 'dW', 'dU', 'db')
    return {n: rel(g, r) for n, g, r in zip(names, got, ref) if r is not None}


def check_layer(errs, label):
    print('%s: %s' % (label, '  '.join('%s %.2e' % kv for kv in errs.items())))
    assert errs['h'] <= FWD and errs['dx'] <= DATA and errs['dW'] <= WEIGHT and errs['dU'] <= WEIGHT and errs.get('db', 0.0) <= WEIGHT, (label, errs)


# a cover of units {1, 7, 32, 100, 128} x Cin {1, 100} x T {1, 2, 97, 384} x N {1, 3, 50}, both cells
COVER = [(1, 1, 1, 1), (1, 100, 2, 3), (7, 1, 97, 3), (7, 100, 384, 1), (32, 1, 2, 50), (32, 100, 97, 1), (100, 1, 384, 3), (100, 100, 97, 50),
         (128, 1, 97, 3), (128, 100, 1, 50), (128, 100, 384, 1)]


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
@pytest.mark.parametrize('u,cin,T,N', COVER)
def test_layer_forward_and_gradients(cell, u, cin, T, N):
    d = layer_data(cell, N, T, cin, u, seed=u + cin + T + N)
    check_layer(layer_errors(gpu_layer(cell, *d), twin_layer(cell, *d)), '%s u=%d Cin=%d T=%d N=%d' % (cell, u, cin, T, N))


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
@pytest.mark.parametrize('kw', [dict(go_backwards=True), dict(rec='hard_sigmoid'), dict(act='sigmoid'), dict(act='relu'), dict(act='linear'),
                                dict(go_backwards=True, rec='hard_sigmoid', act='relu')], ids=lambda k: '-'.join('%s=%s' % kv for kv in k.items()))
def test_layer_options(cell, kw):
    d = layer_data(cell, 3, 61, 5, 20, seed=7)
    check_layer(layer_errors(gpu_layer(cell, *d, **kw), twin_layer(cell, *d, **kw)), '%s %s' % (cell, kw))


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_layer_without_bias_and_on_channel_slices(cell):
    d = layer_data(cell, 3, 50, 4, 33, seed=8, use_bias=False)
    check_layer(layer_errors(gpu_layer(cell, *d), twin_layer(cell, *d)), cell + ' use_bias=False')
    d = layer_data(cell, 3, 50, 4, 33, seed=9)
    check_layer(layer_errors(gpu_layer(cell, *d, sliced=True), twin_layer(cell, *d)), cell + ' strided')


def test_gate_functions_saturate():
    """|x| of 1e4 and more in the projected gates: outputs stay finite and inside the activations' ranges."""
    for cell in ('lstm', 'gru'):
        G = ops.RNN_GATES[cell]
        g = torch.Generator().manual_seed(1)
        zx = ((torch.rand(2, 9, G * 5, generator=g) - 0.5) * 2e4).cuda()
        zx[0, 0, :3] = torch.tensor([float('inf'), -float('inf'), 3e38])
        U = torch.from_numpy(keras_initializer('orthogonal', (5, G * 5), np.random.default_rng(0))).cuda()
        h, saved = ops.rnn_fwd(zx, U, None, cell=cell)
        assert torch.isfinite(h).all() and float(h.abs().max()) <= 1.0
        dzx, dzh = ops.rnn_bwd(U, saved, h, torch.ones_like(h), cell=cell)
        assert torch.isfinite(dzx).all() and torch.isfinite(dzh).all()


@pytest.mark.parametrize('cell,wrong,kw', [('lstm', 'swap_if', {}), ('gru', 'reset_before', {}), ('lstm', 'flip_back', dict(go_backwards=True)),
                                           ('gru', 'flip_back', dict(go_backwards=True))])
def test_layer_sensitivity(cell, wrong, kw):
    """The comparison is not blind: against a deliberately wrong twin every bound it is run under fails."""
    d = layer_data(cell, 3, 61, 5, 20, seed=11)
    errs = layer_errors(gpu_layer(cell, *d, **kw), twin_layer(cell, *d, wrong=wrong, **kw))
    print('%s vs wrong twin %s: %s' % (cell, wrong, errs))
    assert errs['h'] > FWD and errs['dx'] > DATA and errs['dW'] > WEIGHT and errs['dU'] > WEIGHT and errs['db'] > WEIGHT


# ----------------------------------------------------------------------------------------------------------------- whole model
def model_and_data(cfg, N, L, seed=0, **kw):
    m = Dirichlet_BC_RNN(**cfg, seed=seed, **kw)
    rng = np.random.default_rng(seed + 10)
    m.set_weights([w if not n.endswith('/bias') else (w + rng.standard_normal(w.shape) * 0.1).astype(np.float32) for n, w in zip(m.weight_names, m.get_weights())])
    bc = torch.from_numpy((np.cumsum(rng.standard_normal((N, 1, L)), 2) * 0.1).astype(np.float32))
    return m, bc


def params(m, requires_grad=True):
    return {n: torch.from_numpy(w).double().requires_grad_(requires_grad) for n, w in zip(m.weight_names, m.get_weights())}


def flat_grad(m, P):
    return torch.cat([P[n].grad.reshape(-1) for n in m.weight_names])


def model_errors(m, bc, X, wrong=None):
    N = bc.shape[0]
    dx = torch.full((N, 1), 0.02)
    pred = m([bc, dx, X])
    P = params(m)
    ref = TW.forward(m, P, bc.double(), X, wrong=wrong)
    if tuple(ref.shape) != tuple(pred.shape):
        return None, None
    dpred = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).cuda()
    m.backward(dpred)
    ref.mul(dpred.double().cpu()).sum().backward()
    return rel(pred, ref), rel(m.store.flat_g, flat_grad(m, P))


@pytest.mark.parametrize('cell,method', [('lstm', 'bilinear'), ('lstm', 'bicubic'), ('gru', 'bilinear')])
def test_model_at_shipped_depth(cell, method):
    """experiments/dbcnn_rnn.json's six layers of 100 units at T = 384 (the upper end of its shape range), non-square output."""
    cfg = dict(configs.dbcnn_rnn()['model'], RNN_type=cell, resize_method=method)
    m, bc = model_and_data(cfg, 3, 384)
    ef, eg = model_errors(m, bc, 200)
    print('Dirichlet_BC_RNN 6 x 100 %s %s T=384: forward rel-L2 %.3e  flat gradient rel-L2 %.3e' % (cell, method, ef, eg))
    assert ef <= MODEL_FWD and eg <= MODEL_GRAD


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_model_tiny_options_and_sensitivity(cell):
    base = dict(configs.dbcnn_rnn_tiny()['model'], RNN_type=cell.upper())
    for kw in (dict(), dict(go_backwards=True, recurrent_activation='hard_sigmoid'), dict(use_bias=False), dict(data_format='channels_first', activations=['relu', 'sigmoid'])):
        m, bc = model_and_data(dict(base, **{k: v for k, v in kw.items() if k in ('activations', 'data_format')}), 3, 45, seed=2,
                               **{k: v for k, v in kw.items() if k not in ('activations', 'data_format')})
        ef, eg = model_errors(m, bc, 52)
        print('tiny %s %s: forward %.3e gradient %.3e' % (cell, kw, ef, eg))
        assert ef <= MODEL_FWD and eg <= MODEL_GRAD
    # the resize target axes exchanged: on a non-square case the shapes differ; on the exchanged-size case the values do
    m, bc = model_and_data(base, 3, 45, seed=2)
    assert model_errors(m, bc, 52, wrong='swap_axes') == (None, None)
    m2, bc2 = model_and_data(base, 3, 45, seed=2)
    pred = m2([bc2, torch.full((3, 1), 0.02), 52])                                  # (3, 1, 52, 45)
    wrong = TW.forward(m2, params(m2, False), bc2.double(), 52, wrong='swap_axes')   # (3, 1, 45, 52)
    assert rel(pred, wrong.transpose(2, 3)) > MODEL_FWD
    # channels_last is the same memory
    m3 = Dirichlet_BC_RNN(**dict(base, data_format='channels_last'), seed=2)
    m3.set_weights(m.get_weights())
    y3 = m3([bc.permute(0, 2, 1), torch.full((3, 1), 0.02), 52])
    assert tuple(y3.shape) == (3, 52, 45, 1) and torch.equal(y3.reshape(3, 1, 52, 45), m([bc, torch.full((3, 1), 0.02), 52]))


def compiled(cfg_full, N, seed=0, max_input_shape=None, lr=1e-3):
    m = Dirichlet_BC_RNN(**cfg_full['model'], seed=seed)
    m.compile(loss=loss_wrapper(global_batch_size=N, **cfg_full['training']['loss_parameters']), optimizer=Adam(learning_rate=lr), max_input_shape=max_input_shape)
    return m


def batch(N, X, L, seed):
    rng = np.random.default_rng(seed)
    bc = torch.from_numpy((np.cumsum(rng.standard_normal((N, 1, L)), 2) * 0.1).astype(np.float32))
    y = torch.from_numpy(rng.uniform(-0.5, 0.5, (N, 1, X, L)).astype(np.float32))
    return (bc, torch.full((N, 1), 0.02)), y


def test_route_one_recurrence_launch_per_layer_and_direction(monkeypatch):
    """A train step calls ops.rnn_fwd and ops.rnn_bwd once per layer whatever T is (each is one kernel launch), and the number of all libpcnn
    launches does not depend on T either: nothing runs per time step."""
    full = configs.dbcnn_rnn_tiny()
    full['model']['units'] = [12, 9, 5]
    counts = {}
    for T in (24, 131):
        m = compiled(full, 2)
        n = {'fwd': 0, 'bwd': 0, 'calls': 0}
        rf, rb, real_call = ops.rnn_fwd, ops.rnn_bwd, type(ops.handle()).call

        def fwd(*a, **k):
            n['fwd'] += 1
            return rf(*a, **k)

        def bwd(*a, **k):
            n['bwd'] += 1
            return rb(*a, **k)

        def call(self, name, *a):
            n['calls'] += 1
            return real_call(self, name, *a)
        monkeypatch.setattr(ops, 'rnn_fwd', fwd)
        monkeypatch.setattr(ops, 'rnn_bwd', bwd)
        monkeypatch.setattr(type(ops.handle()), 'call', call)
        m.train_step(batch(2, 40, T, 1))
        monkeypatch.undo()
        counts[T] = dict(n)
    assert counts[24]['fwd'] == counts[24]['bwd'] == 3 and counts[131]['fwd'] == counts[131]['bwd'] == 3
    assert counts[24]['calls'] == counts[131]['calls'], counts


def test_steps_are_deterministic_and_presized():
    full = configs.dbcnn_rnn_tiny()
    big, small = (48, 56), (40, 44)                                              # (X, L)
    data_big, data_small = batch(2, *big, 1), batch(2, *small, 2)
    a = compiled(full, 2, max_input_shape=(2,) + big)
    b = compiled(full, 2, max_input_shape=(2,) + big)
    a.train_step(data_big)
    b.train_step(data_big)
    assert torch.equal(a.store.flat_w, b.store.flat_w)                           # two identical steps: bit-identical weights (no atomics)
    # per-shape constants (resize and quadrature tables) are cached by ops / the loss for every model; build those of the new shape outside the
    # measured step, so that what is measured is the model's own buffers
    c = compiled(full, 2)
    c.train_step(data_small)                                                     # ops' resize tables (process-wide)
    ys = data_small[1].cuda()
    a.loss_fn.value_and_grad(ys, torch.zeros_like(ys), torch.zeros_like(ys), torch.full((2, 2), 0.02, device='cuda'))   # the loss object's quadrature vectors
    del ys
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    arena = a._arena.data_ptr()
    a.train_step(data_small)                                                     # a step after a shape change
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and a._arena.data_ptr() == arena
    fresh = compiled(full, 2)
    fresh.set_weights(b.get_weights())
    fresh.optimizer.iterations = b.optimizer.iterations
    fresh.optimizer.ms[0].copy_(b.optimizer.ms[0])
    fresh.optimizer.vs[0].copy_(b.optimizer.vs[0])
    fresh.train_step(data_small)
    assert torch.equal(fresh.store.flat_w, a.store.flat_w)                       # ... and equals the same step in a fresh model


def test_two_adam_steps_against_the_twin():
    full = configs.dbcnn_rnn_tiny()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-7
    m = compiled(full, 2, lr=lr)
    w = {n: torch.from_numpy(v).double() for n, v in zip(m.weight_names, m.get_weights())}
    w0 = torch.cat([w[n].reshape(-1) for n in m.weight_names])
    mom = torch.zeros_like(w0)
    var = torch.zeros_like(w0)
    flat = w0.clone()
    for step in (1, 2):
        (bc, dx), y = batch(2, 44, 50, 20 + step)
        pred = m.call([bc, dx, 44])
        _, dpred = m.loss_fn.value_and_grad(y.cuda(), pred, torch.zeros_like(y).cuda(), torch.cat([dx, dx], 1).cuda())
        P, off = {}, 0
        for n in m.weight_names:
            k = w[n].numel()
            P[n] = flat[off:off + k].reshape(w[n].shape).clone().requires_grad_(True)
            off += k
        TW.forward(m, P, bc.double(), 44).mul(dpred.double().cpu()).sum().backward()
        g = flat_grad(m, P)
        mom = b1 * mom + (1 - b1) * g
        var = b2 * var + (1 - b2) * g * g
        flat = flat - lr * np.sqrt(1 - b2 ** step) / (1 - b1 ** step) * mom / (var.sqrt() + eps)
        logs = m.train_step(((bc, dx), y))
        assert set(logs) == {'loss', 'mse', 'lr'}
        got = m.store.flat_w.double().cpu()
        sel = g.abs() > 1e-2 * g.abs().max()
        e = rel((got - w0)[sel], (flat - w0)[sel])
        print('Adam step %d: update rel-L2 vs twin %.3e' % (step, e))
        assert e <= 3e-3


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_train_cli_two_epochs_and_checkpoint(tmp_path, fmt):
    cfg = configs.dbcnn_rnn_tiny()
    p = tmp_path / 'dbcnn_rnn.json'
    configs.dump_config(cfg, str(p))
    r = subprocess.run([sys.executable, '-m', 'poisson_cnn_amd.train', str(p), '--model', 'dbcnn_rnn', '--epochs', '2', '--checkpoint_dir', str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'Dirichlet_BC_RNN' in r.stdout
    m = Dirichlet_BC_RNN(**cfg['model'], seed=5)
    before = m.store.flat_w.clone()
    m.load_weights(str(tmp_path / 'chkpt.checkpoint.npz'))
    assert not torch.equal(m.store.flat_w, before)
    if fmt == 'tf':
        m.save_weights(str(tmp_path / 'again'), save_format='tf')
        m2 = Dirichlet_BC_RNN(**cfg['model'], seed=6)
        m2.load_weights(str(tmp_path / 'again'))
        assert torch.equal(m2.store.flat_w, m.store.flat_w)
    (bc, dx), _ = batch(2, 40, 44, 3)
    assert torch.isfinite(m([bc, dx, 40])).all()


def test_graphed_train_step_replays_bit_identically():
    from poisson_cnn_amd.graphs import GraphedTrainStep
    full = configs.dbcnn_rnn_tiny()
    data = batch(2, 40, 44, 4)
    eager, graphed = compiled(full, 2), compiled(full, 2)
    step = GraphedTrainStep(graphed, data)
    for k in range(2):
        d = batch(2, 40, 44, 5 + k)
        le, lg = eager.train_step(d), step(d)
        assert torch.equal(eager.store.flat_w, graphed.store.flat_w)
        assert float(le['loss']) == float(lg['loss'])
    step.close()
