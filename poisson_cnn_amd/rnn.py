"""Dirichlet_BC_RNN (models/Dirichlet_BC_RNN.py:7-81; experiments/dbcnn_rnn.json, train/dbcnn_rnn_train.py): a stack of LSTM or GRU layers run
along the boundary, whose (N, L, units) output is read as a one-channel image and resized to the domain by the Upsample layer.

    model([bc (N,1,L), dx (N,1), x_output_resolution]) -> (N,1,X,L);   compile(loss, optimizer[, max_input_shape]);   train_step(((bc, dx), y))

Built AS WRITTEN (:38-58): bc is transposed to (N, L, 1) so that L is the time axis; the stack's output (N, L, u_last) becomes an image of
L x u_last pixels and is resized to (x_output_resolution, L) - the unit axis is stretched over the boundary axis and the time axis over X.
`domain_sizes` is computed by the reference but unused by Upsample at ndims = 2.

Every layer is two kinds of launches (csrc/rnn.hip): the time-parallel products (x W + b for all t; dX, dW, dU, db) are 1x1 convolutions over all
rows on the wide-convolution kernels, and the dependent chain over t is ONE persistent-kernel launch per layer and direction (ops.rnn_fwd / rnn_bwd).
Sequences live in buffers of T + 1 rows per sample: activations h_t in row t + 1 behind a zero row, gradients dZ_t in row t before a zero row.  Read
as flat row lists, h_{t-1} then pairs with dZ_t row by row and x_t with dZ_t after a shift by one row, so dU and dW are each one wgrad call over all
N (T + 1) rows; the zero rows make the pairs across sample borders vanish.
There is no TensorFlow here: PARITY UNPINNED, checked against the fp64 restatement of the Keras equations in tests/rnn_twin.py.
"""
import numpy as np
import torch

from . import layers as L
from . import ops
from .models import _CPU_NOTE, _ModelBase, _as_device, _dx_column, _dx_pair

_RNN_ACTS = {'tanh': 'tanh', 'tf.nn.tanh': 'tanh', 'tf.math.tanh': 'tanh', 'tf.keras.activations.tanh': 'tanh',
             'sigmoid': 'sigmoid', 'tf.nn.sigmoid': 'sigmoid', 'tf.math.sigmoid': 'sigmoid', 'tf.keras.activations.sigmoid': 'sigmoid',
             'relu': 'relu', 'tf.nn.relu': 'relu', 'tf.keras.activations.relu': 'relu',
             'linear': 'linear', 'tf.keras.activations.linear': 'linear', None: 'linear'}
_REC_ACTS = {'sigmoid': 'sigmoid', 'tf.nn.sigmoid': 'sigmoid', 'tf.math.sigmoid': 'sigmoid', 'tf.keras.activations.sigmoid': 'sigmoid',
             'hard_sigmoid': 'hard_sigmoid', 'tf.keras.activations.hard_sigmoid': 'hard_sigmoid'}
_INITIALIZERS = ('glorot_uniform', 'orthogonal', 'zeros', 'ones')
# keyword arguments of tf.keras.layers.LSTM / GRU that are accepted only at the one value the kernels implement
_FIXED = {'dropout': 0, 'recurrent_dropout': 0, 'stateful': False, 'unroll': False, 'return_state': False}
_ACCEPTED = ('recurrent_activation', 'use_bias', 'unit_forget_bias', 'go_backwards', 'kernel_initializer', 'recurrent_initializer', 'bias_initializer',
             'reset_after', 'implementation') + tuple(_FIXED)


def _name(v, table, what):
    if callable(v):
        raise NotImplementedError('%s: a callable is not implemented, pass a name (%s)' % (what, sorted(k for k in table if k and '.' not in k)))
    key = v.lower() if isinstance(v, str) else v
    if key not in table:
        raise ValueError('%s: unsupported value %r' % (what, v))
    return table[key]


def keras_initializer(name, shape, rng):
    """glorot_uniform / orthogonal / zeros / ones as tf.keras.initializers draws them (values from this library's own generator)."""
    if name == 'glorot_uniform':
        lim = float(np.sqrt(6.0 / (shape[0] + shape[-1])))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)
    if name == 'orthogonal':            # tf.keras.initializers.Orthogonal: QR of a (max, min) normal matrix, signs fixed by diag(R), transposed when wide
        rows, cols = int(np.prod(shape[:-1])), int(shape[-1])
        q, r = np.linalg.qr(rng.standard_normal((max(rows, cols), min(rows, cols))))
        q = q * np.sign(np.diag(r))
        if rows < cols:
            q = q.T
        return np.ascontiguousarray(q.reshape(shape), dtype=np.float32)
    if name == 'zeros':
        return np.zeros(shape, dtype=np.float32)
    if name == 'ones':
        return np.ones(shape, dtype=np.float32)
    raise NotImplementedError(name)


class Dirichlet_BC_RNN(_ModelBase):
    model_name = 'Dirichlet_BC_RNN'

    def __init__(self, units, activations='tanh', RNN_type='lstm', resize_method='bicubic', data_format='channels_first', device=None, seed=0, **rnn_args):
        if data_format not in ('channels_first', 'channels_last'):
            raise ValueError('data_format must be channels_first or channels_last')
        if not isinstance(RNN_type, str):
            raise NotImplementedError('RNN_type: a layer class is not implemented, pass "lstm" or "gru"')
        self.cell = RNN_type.lower()
        if self.cell not in ops.RNN_CELLS:
            raise KeyError(RNN_type)                                            # the reference's dict lookup (:21)
        self.units = [int(v) for v in units]
        n_layers = len(self.units)
        if n_layers < 1:
            raise ValueError('units must name at least one layer')
        for v in self.units:
            if not 1 <= v <= ops.RNN_MAX_UNITS:
                raise NotImplementedError('units = %d: the recurrence kernels keep a layer\'s recurrent kernel in registers and are built for 1 <= units <= %d'
                                          % (v, ops.RNN_MAX_UNITS))
        if callable(activations) or isinstance(activations, str) or activations is None:
            activations = [activations] * n_layers
        self.acts = [_name(a, _RNN_ACTS, 'activations') for a, _ in zip(activations, self.units)]
        if len(self.acts) != n_layers:                                         # the reference's zip() would silently build fewer layers (:27)
            raise ValueError('activations names %d layers, units %d' % (len(self.acts), n_layers))
        for k, v in rnn_args.items():
            if k not in _ACCEPTED:
                raise NotImplementedError('Dirichlet_BC_RNN: the recurrent-layer argument %r is not implemented' % k)
            if k in _FIXED and v != _FIXED[k]:
                raise NotImplementedError('Dirichlet_BC_RNN: %s=%r is not implemented (only %r)' % (k, v, _FIXED[k]))
        if self.cell == 'gru' and not rnn_args.get('reset_after', True):
            raise NotImplementedError('Dirichlet_BC_RNN: reset_after=False is not implemented (the TF 2 default reset_after=True is)')
        if self.cell == 'lstm' and 'reset_after' in rnn_args:
            raise NotImplementedError('Dirichlet_BC_RNN: reset_after is an argument of the GRU only')
        self.rec_act = _name(rnn_args.get('recurrent_activation', 'sigmoid'), _REC_ACTS, 'recurrent_activation')
        self.use_bias = bool(rnn_args.get('use_bias', True))
        self.unit_forget_bias = bool(rnn_args.get('unit_forget_bias', True))
        self.go_backwards = bool(rnn_args.get('go_backwards', False))
        inits = {}
        for k, default in (('kernel_initializer', 'glorot_uniform'), ('recurrent_initializer', 'orthogonal'), ('bias_initializer', 'zeros')):
            v = rnn_args.get(k, default)
            if not isinstance(v, str) or v.lower() not in _INITIALIZERS:
                raise NotImplementedError('Dirichlet_BC_RNN: %s=%r is not implemented (by name: %s)' % (k, v, ', '.join(_INITIALIZERS)))
            inits[k] = v.lower()
        if resize_method not in ops.RESIZE:
            raise ValueError('resize_method must be one of %s' % sorted(ops.RESIZE))
        self._init_device(device, _CPU_NOTE)
        self.data_format, self.resize_method = data_format, resize_method
        self.G = G = ops.RNN_GATES[self.cell]
        self.store = S = L.ParamStore()
        self.ctx = L.Context()
        # Keras names: lstm[_n]/lstm_cell[_n]/{kernel, recurrent_kernel, bias}
        self.layers = []                                                       # (kernel, recurrent_kernel, bias or None, Cin, units, activation)
        cin = 1
        for i, (u, act) in enumerate(zip(self.units, self.acts)):
            sfx = '_%d' % i if i else ''
            base = '%s%s/%s_cell%s' % (self.cell, sfx, self.cell, sfx)
            kn = S.add(base + '/kernel', (cin, G * u), 'zeros')
            rn = S.add(base + '/recurrent_kernel', (u, G * u), 'zeros')
            bn = S.add(base + '/bias', (G * u,) if self.cell == 'lstm' else (2, G * u), 'zeros') if self.use_bias else None
            self.layers.append((kn, rn, bn, cin, u, act))
            cin = u
        S.finalize(self.device)
        S.initialize(seed)
        rng = np.random.default_rng(seed + 1)
        for kn, rn, bn, cin, u, _ in self.layers:
            S.w[kn].copy_(torch.from_numpy(keras_initializer(inits['kernel_initializer'], (cin, G * u), rng)))
            S.w[rn].copy_(torch.from_numpy(keras_initializer(inits['recurrent_initializer'], (u, G * u), rng)))
            if bn is not None:
                b = keras_initializer(inits['bias_initializer'], tuple(S.w[bn].shape), rng)
                if self.cell == 'lstm' and self.unit_forget_bias:              # Keras: [bias_initializer(u) | ones(u) | bias_initializer(2u)]
                    b[u:2 * u] = 1.0
                S.w[bn].copy_(torch.from_numpy(b))
        self._arena = None
        self._saved = None

    # ------------------------------------------------------------------ buffers
    def _plan(self, N, T):
        """name -> (offset, floats) of every sequence buffer of one forward + backward at (N, T), and their total."""
        R = N * (T + 1)
        G = self.G
        umax, cmax = max(self.units), max([1] + self.units[:-1])
        plan, off = {}, 0

        def take(name, n):
            nonlocal off
            plan[name] = (off, n)
            off += (n + 63) // 64 * 64

        take('x0', R + 1)
        take('zx', R * G * umax)
        for i, u in enumerate(self.units):
            take('h%d' % i, (R + 1) * u)
            take('saved%d' % i, N * T * (G + 1) * u)
        take('out', N * T * self.units[-1])
        take('dzx', R * G * umax)
        take('dzh', R * G * umax)
        take('dh0', R * cmax)
        take('dh1', R * cmax)
        take('wt', G * umax * cmax)
        return plan, off

    def _buffers(self, N, T):
        plan, total = self._plan(N, T)
        if self._arena is None or self._arena.numel() < total:
            self._arena = None
            self._arena = torch.empty(total, dtype=torch.float32, device=self.device)
        return {k: self._arena[o:o + n] for k, (o, n) in plan.items()}

    # ------------------------------------------------------------------ forward (:38-58)
    def call(self, inp, training=False):
        bc, dx, X = inp
        X = int(X)
        bc = _as_device(bc, self.device)
        if bc.dim() != 3 or bc.shape[1] != 1:
            raise ValueError('bc must have shape (N,1,L)')
        N, _, T = bc.shape
        R = N * (T + 1)
        G, S = self.G, self.store
        B = self._buffers(N, T)
        as4 = lambda flat, C, first=0: flat[first * C:(first + R) * C].view(1, T + 1, N, C)          # noqa: E731
        x = B['x0']
        x3 = x[:R].view(N, T + 1, 1)
        x3[:, 0].zero_()
        x[R:].zero_()
        x3[:, 1:, 0].copy_(bc[:, 0, :])                                          # tf.transpose(bc, [0, 2, 1]): L becomes the time axis
        hs = []
        last = len(self.layers) - 1
        for i, (kn, rn, bn, cin, u, act) in enumerate(self.layers):
            Gu = G * u
            zx = B['zx'][:R * Gu]
            bias = None if bn is None else (S.w[bn] if self.cell == 'lstm' else S.w[bn][0])
            ops.wide_conv2d_fwd(as4(x, cin, 1), S.w[kn].view(1, 1, cin, Gu), bias, out=zx.view(1, T + 1, N, Gu))
            h = B['h%d' % i]
            h3 = h[:R * u].view(N, T + 1, u)
            h3[:, 0].zero_()
            h[R * u:].zero_()
            h2 = B['out'].view(N, T, u) if i == last else None
            ops.rnn_fwd(zx.view(N, T + 1, Gu)[:, :T], S.w[rn], None if (bn is None or self.cell == 'lstm') else S.w[bn][1], cell=self.cell, act=act,
                        rec_act=self.rec_act, reverse=self.go_backwards, h=h3[:, 1:], h2=h2, saved=B['saved%d' % i])
            hs.append(h)
            x = h
        u = self.units[-1]
        img = B['out'].view(N, T, u, 1)                                          # tf.expand_dims: (N, L, u_last) is the one-channel image, no copy
        y = ops.resize_fwd(img, (X, T), self.resize_method)                      # Upsample([out, domain_sizes, (X, L)]) (:54)
        self._saved = {'N': N, 'T': T, 'X': X, 'B': B}
        return y.view(N, 1, X, T)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred, need_dx=False):
        """Gradient of every parameter (into store.flat_g) from dL/dpred (N,1,X,L); returns dL/dbc (N,1,L) if need_dx."""
        sv = self._saved
        if sv is None:
            raise RuntimeError('Dirichlet_BC_RNN.backward() without a preceding call()')
        self._saved = None
        N, T, X, B = sv['N'], sv['T'], sv['X'], sv['B']
        R = N * (T + 1)
        G, S, g, ws = self.G, self.store, self.store.g, self.ctx.ws
        as4 = lambda flat, C, first=0: flat[first * C:(first + R) * C].view(1, T + 1, N, C)          # noqa: E731
        dpred = _as_device(dpred, self.device).contiguous().view(N, X, T, 1)
        u = self.units[-1]
        dh = ops.resize_bwd(dpred, (T, u), self.resize_method).view(N, T, u)
        dbc = None
        for i in range(len(self.layers) - 1, -1, -1):
            kn, rn, bn, cin, u, act = self.layers[i]
            Gu = G * u
            x = B['h%d' % (i - 1)] if i > 0 else B['x0']
            h = B['h%d' % i]
            dzx = B['dzx'][:R * Gu]
            one = self.cell == 'lstm' and not self.go_backwards
            dzh = dzx if one else B['dzh'][:R * Gu]
            dzx.view(N, T + 1, Gu)[:, T].zero_()
            if not one:
                dzh.view(N, T + 1, Gu)[:, T].zero_()
            ops.rnn_bwd(S.w[rn], B['saved%d' % i], h[:R * u].view(N, T + 1, u)[:, 1:], dh, cell=self.cell, act=act, rec_act=self.rec_act,
                        reverse=self.go_backwards, dzx=dzx.view(N, T + 1, Gu)[:, :T], dzh=dzh.view(N, T + 1, Gu)[:, :T])
            dzx4, dzh4 = dzx.view(1, T + 1, N, Gu), dzh.view(1, T + 1, N, Gu)
            db_x = None if bn is None else (g[bn] if self.cell == 'lstm' else g[bn][0])
            db_h = None if (bn is None or self.cell == 'lstm') else g[bn][1]
            ops.wide_conv2d_wgrad(as4(x, cin, 1), dzx4, (1, 1, cin, Gu), dw=g[kn].view(1, 1, cin, Gu), dbias=db_x, ws=ws)       # dW = sum_t x_t^T dZ_t
            ops.wide_conv2d_wgrad(as4(h, u, 0), dzh4, (1, 1, u, Gu), dw=g[rn].view(1, 1, u, Gu), dbias=db_h, ws=ws)           # dU = sum_t h_{t-1}^T dZ_t
            if i > 0 or need_dx:
                wt = ops.flip_transpose_weights(S.w[kn].view(1, 1, cin, Gu), out=B['wt'][:Gu * cin].view(1, 1, Gu, cin))
                dxb = B['dh%d' % (i & 1)][:R * cin]
                ops.wide_conv2d_dgrad(dzx4, wt, out=dxb.view(1, T + 1, N, cin))                                               # dX = dZ W^T
                dh = dxb.view(N, T + 1, cin)[:, :T]
                if i == 0:
                    dbc = dh.reshape(N, 1, T).clone()
        return dbc

    # ------------------------------------------------------------------ training (:60-75)
    def _dummy_batch(self, shape):
        N, H, W = shape
        gen = torch.Generator(device='cpu').manual_seed(0)
        bc = torch.cumsum(torch.randn((N, 1, W), generator=gen), 2) * 0.1
        return (bc.to(self.device), torch.full((N, 1), 0.02, device=self.device)), (torch.rand((N, 1, H, W), generator=gen) * 0.1).to(self.device)

    def _forward_backward(self, data):
        (bc, dx), y_true = data
        bc, dx, y_true = _as_device(bc, self.device), _as_device(dx, self.device), _as_device(y_true, self.device)
        dx = _dx_column(dx)
        pred = self.call([bc, dx, y_true.shape[2]], training=True)                # x_output_resolution from the target's shape (:64)
        loss, dpred = self.loss_fn.value_and_grad(y_true, pred, torch.zeros_like(y_true), _dx_pair(dx))
        self.backward(dpred)
        return loss, y_true, pred
