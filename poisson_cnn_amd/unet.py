"""The UNet baseline (models/UNet.py:188-267 + UNetModel.train_step :166-182) on the wide-channel libpcnn kernels (csrc/conv_wide.hip).

`UNet(**config['model'])` takes the reference's signature (experiments/UNet.json loads unchanged) and returns a model with the Keras-style weight
API of the other models (one ParamStore: Adam, grad_sync / DataParallel, save_weights / load_weights, get_weights / set_weights, summary).
`model(rhs, training=False)` takes the RHS alone, (N, in_channels, H, W) channels_first as the reference's training script sets it, and returns
(N, out_channels, H, W).  Inside, data is NHWC; every level's concat buffer [skip | upsampled] is written in place by the convolution and the
transposed convolution that produce its halves, so no concat copy exists.
"""
import numpy as np
import torch

from . import layers as L
from . import ops
from .models import _CPU_NOTE, _ModelBase, _as_device, _dx_column, _dx_pair
from .utils import canonical_activation


def _filters(i, root):
    return 2 ** i * root


def _trunc_std(filters, k):
    """models/UNet.py:32-34"""
    return float(np.sqrt(2.0 / (k ** 2 * filters)))


class UNetModel(_ModelBase):
    model_name = 'unet'

    def __init__(self, nx=None, ny=None, in_channels=1, out_channels=1, layer_depth=5, filters_root=64, kernel_size=3, pool_size=2,
                 dropout_rate=0.5, padding='valid', activation='relu', final_activation='linear', device=None, seed=0):
        if str(padding).lower() != 'same':
            raise NotImplementedError("UNet(padding=%r): only padding='same' is implemented (experiments/UNet.json); with 'valid' the output "
                                      "shrinks and the reference's own loss_wrapper cannot compare it with the target" % (padding,))
        if kernel_size % 2 != 1 or kernel_size > 7:
            raise NotImplementedError('UNet: kernel_size must be odd and <= 7 (the wide convolution kernels), got %r' % (kernel_size,))
        if pool_size not in (2, 3):
            raise NotImplementedError('UNet: pool_size must be 2 or 3, got %r' % (pool_size,))
        if layer_depth < 2:
            raise ValueError('UNet: layer_depth must be >= 2')
        if canonical_activation(final_activation) != 'linear':
            raise NotImplementedError('UNet: final_activation other than linear is not implemented')
        self._init_device(device, _CPU_NOTE, name='UNet')
        self.nx, self.ny = nx, ny
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.depth, self.root, self.k, self.pool = int(layer_depth), int(filters_root), int(kernel_size), int(pool_size)
        self.dropout_rate = float(dropout_rate)
        self.act = canonical_activation(activation)
        self.store = S = L.ParamStore()
        self.ctx = L.Context()
        # Keras construction order and names: ConvBlock(i) -> conv_block[_n]/conv2d[_m], deconvupscale[_n], the 1x1 head conv2d_m
        self._trunc = {}
        self.convs = []                                                    # (kernel name, bias name, cin, cout, k)
        nconv = [0]
        nblock = [0]

        def conv(block, cin, cout, k, std):
            idx = nconv[0]
            nconv[0] += 1
            base = '%sconv2d%s' % (block + '/' if block else '', '_%d' % idx if idx else '')
            kn = S.add(base + '/kernel', (k, k, cin, cout), 'zeros')
            bn = S.add(base + '/bias', (cout,), 'zeros')
            self._trunc[kn] = std
            return (kn, bn, cin, cout, k)

        def conv_block(i, cin):
            b = nblock[0]
            nblock[0] += 1
            name = 'conv_block' + ('_%d' % b if b else '')
            F = _filters(i, self.root)
            std = _trunc_std(F, self.k)
            return (conv(name, cin, F, self.k, std), conv(name, F, F, self.k, std))

        self.down = []
        cin = self.in_channels
        for i in range(self.depth - 1):
            self.down.append(conv_block(i, cin))
            cin = _filters(i, self.root)
        self.bottom = conv_block(self.depth - 1, cin)
        self.up = []
        prev = _filters(self.depth - 1, self.root)
        for j, i in enumerate(range(self.depth - 2, -1, -1)):
            F = _filters(i + 1, self.root) // 2
            name = 'deconvupscale' + ('_%d' % j if j else '')
            dk = S.add(name + '/kernel', (self.pool, self.pool, F, prev), 'glorot')
            db = S.add(name + '/bias', (F,), 'glorot')
            blk = conv_block(i, F + _filters(i, self.root))
            self.up.append(((dk, db, prev, F), blk))
            prev = _filters(i, self.root)
        self.head = conv('', prev, self.out_channels, 1, _trunc_std(self.root, self.k))
        S.finalize(self.device)
        S.initialize(seed)
        rng = np.random.default_rng(seed + 1)
        for name, std in self._trunc.items():                            # TruncatedNormal(stddev): normal re-drawn outside 2 sigma
            shape = S.w[name].shape
            v = rng.standard_normal(int(np.prod(shape)))
            bad = np.abs(v) > 2.0
            while bad.any():
                v[bad] = rng.standard_normal(int(bad.sum()))
                bad = np.abs(v) > 2.0
            S.w[name].copy_(torch.from_numpy((v * std).astype(np.float32).reshape(tuple(shape))))
        self._acc = None
        self._saved = None
        self._drop_calls = 0
        self._seed = int(seed)

    # ------------------------------------------------------------------ forward
    def _drop(self, training, layer_id):
        if not training or self.dropout_rate <= 0.0:
            return None
        return (self.dropout_rate, self._call_seed, layer_id)

    def _conv(self, spec, x, training, lid, out=None, act=None):
        kn, bn, _, _, _ = spec
        S = self.store
        return ops.wide_conv2d_fwd(x, S.w[kn], S.w[bn], act=act or self.act, dropout=self._drop(training, lid), out=out)

    def call(self, rhs, training=False):
        """models/UNet.py:212-267.  rhs (N, in_channels, H, W) -> (N, out_channels, H, W) torch CUDA tensor.  training=True applies the ConvBlocks'
        dropout (Keras inverted dropout at dropout_rate); every call keeps what backward() needs."""
        if isinstance(rhs, (list, tuple)):
            raise TypeError('UNet takes the RHS tensor alone (models/UNet.py:172 `self(rhses)`), not a list')
        x = _as_device(rhs, self.device)
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError('rhs must have shape (N, %d, H, W), got %s' % (self.in_channels, tuple(x.shape)))
        N, _, H, W = x.shape
        x = x.reshape(N, H, W, 1) if self.in_channels == 1 else x.permute(0, 2, 3, 1).contiguous()
        dev = x.device
        self._drop_calls += 1
        self._call_seed = (self._seed * 1000003 + self._drop_calls) & 0xFFFFFFFF
        p, Fr = self.pool, self.root
        sizes = [(H, W)]
        for _ in range(self.depth - 1):
            h, w = sizes[-1]
            sizes.append((ops.pool_out(h, p), ops.pool_out(w, p)))
        sv = {'x': x, 'sizes': sizes, 'training': training, 'seed': self._call_seed, 'cat': [], 'a1': [], 'pin': [x], 'e1': [], 'e2': []}
        lid = 0
        inp = x
        for i, (c1, c2) in enumerate(self.down):
            h, w = sizes[i]
            F = _filters(i, Fr)
            cat = ops.empty((N, h, w, 2 * F), dev)
            a1 = self._conv(c1, inp, training, lid)
            self._conv(c2, a1, training, lid + 1, out=cat[..., :F])
            lid += 2
            inp = ops.pool2d_fwd(cat[..., :F], p, 'max')
            sv['cat'].append(cat)
            sv['a1'].append(a1)
            sv['pin'].append(inp)
        b1 = self._conv(self.bottom[0], inp, training, lid)
        b2 = self._conv(self.bottom[1], b1, training, lid + 1)
        sv['b'] = (b1, b2)
        lid += 2
        prev = b2
        for j, ((dk, db, _, F), (c1, c2)) in enumerate(self.up):
            i = self.depth - 2 - j
            h, w = sizes[i]
            cat = sv['cat'][i]
            ops.wide_deconv_fwd(prev, self.store.w[dk], self.store.w[db], (h, w), p, act=self.act, out=cat[..., F:])
            e1 = self._conv(c1, cat, training, lid)
            e2 = self._conv(c2, e1, training, lid + 1)
            lid += 2
            sv['e1'].append(e1)
            sv['e2'].append(e2)
            prev = e2
        y = self._conv(self.head, prev, False, 0)                           # head: conv 1x1 -> Activation(activation) -> linear (:260-267)
        sv['y'] = y
        self._saved = sv
        return y.reshape(N, 1, H, W) if self.out_channels == 1 else y.permute(0, 3, 1, 2).contiguous()

    def __call__(self, rhs, training=False):
        return self.call(rhs, training=training)

    # ------------------------------------------------------------------ backward
    def _flip(self, kn):
        return ops.flip_transpose_weights(self.store.w[kn])

    def _drop_of(self, lid):
        sv = self._saved
        if not sv['training'] or self.dropout_rate <= 0.0:
            return None
        return (self.dropout_rate, sv['seed'], lid)

    def _act_bwd_raw(self, draw, a, lid, out):
        """dz = draw * act'(a) [* dropout mask / (1 - rate)] where draw is a raw gradient at a ConvBlock output (the skip half after the pool
        gradient has been added).  With ReLU the mask is implied by a > 0."""
        ops.epilogue_bwd(draw, a, act=self.act, dz=out, ws=self.ctx.ws)
        d = self._drop_of(lid)
        if d is not None:
            if self.act != 'relu':
                raise NotImplementedError('UNet: dropout (training=True) with a non-ReLU activation is differentiated only inside the fused epilogues')
            ops.axpby(1.0 / (1.0 - self.dropout_rate), out, 0.0, out)
        return out

    def backward(self, dpred, need_dx=True):
        """Gradient of every parameter (into store.flat_g) from dL/dpred (N, out_channels, H, W); returns dL/drhs (None if not need_dx)."""
        sv = self._saved
        if sv is None:
            raise RuntimeError('UNet.backward() without a preceding call()')
        S, g, ws = self.store, self.store.g, self.ctx.ws
        N, H, W = sv['x'].shape[:3]
        dpred = _as_device(dpred, self.device)
        dpred = dpred.reshape(N, H, W, 1) if self.out_channels == 1 else dpred.permute(0, 2, 3, 1).contiguous()
        p, Fr, D = self.pool, self.root, self.depth
        y = sv['y']
        lid_of_block = lambda i: 2 * i                                     # noqa: E731  contracting block i: layers 2i, 2i+1
        lid_up = lambda j: 2 * D + 2 * j                                   # noqa: E731  expanding block j (after the bottom's 2(D-1), 2(D-1)+1)
        # head
        kn, bn, _, _, _ = self.head
        dz = ops.empty(y.shape, y.device)
        ops.epilogue_bwd(dpred, y, act=self.act, dz=dz, ws=ws)
        top = sv['e2'][-1]
        ops.wide_conv2d_wgrad(top, dz, S.w[kn].shape, dw=g[kn], dbias=g[bn], ws=ws)
        dz = ops.wide_conv2d_dgrad(dz, self._flip(kn), act_out=top, act=self.act, dropout=self._drop_of(lid_up(D - 2) + 1))
        # expanding path, from the top level down
        dcats = {}
        for j in range(D - 2, -1, -1):
            (dk, db, _, F), (c1, c2) = self.up[j]
            i = D - 2 - j
            cat, e1 = sv['cat'][i], sv['e1'][j]
            ops.wide_conv2d_wgrad(e1, dz, S.w[c2[0]].shape, dw=g[c2[0]], dbias=g[c2[1]], ws=ws)
            dz = ops.wide_conv2d_dgrad(dz, self._flip(c2[0]), act_out=e1, act=self.act, dropout=self._drop_of(lid_up(j)))
            ops.wide_conv2d_wgrad(cat, dz, S.w[c1[0]].shape, dw=g[c1[0]], dbias=g[c1[1]], ws=ws)
            dcat = ops.wide_conv2d_dgrad(dz, self._flip(c1[0]))          # raw: the skip half still waits for the pool gradient
            dcats[i] = dcat
            dup = ops.empty((N, cat.shape[1], cat.shape[2], F), cat.device)
            ops.epilogue_bwd(dcat[..., F:], cat[..., F:], act=self.act, dz=dup, dbias=g[db], ws=ws)
            prev = sv['e2'][j - 1] if j > 0 else sv['b'][1]
            prev_lid = lid_up(j - 1) + 1 if j > 0 else lid_of_block(D - 1) + 1
            ops.wide_deconv_bwd_filter(prev, dup, p, dk=g[dk], ws=ws)
            dz = ops.wide_deconv_bwd_data(dup, S.w[dk], (prev.shape[1], prev.shape[2]), p, act_out=prev, act=self.act, dropout=self._drop_of(prev_lid))
        # bottom
        b1, b2 = sv['b']
        c1, c2 = self.bottom
        pin = sv['pin'][D - 1]
        ops.wide_conv2d_wgrad(b1, dz, S.w[c2[0]].shape, dw=g[c2[0]], dbias=g[c2[1]], ws=ws)
        dz = ops.wide_conv2d_dgrad(dz, self._flip(c2[0]), act_out=b1, act=self.act, dropout=self._drop_of(lid_of_block(D - 1)))
        ops.wide_conv2d_wgrad(pin, dz, S.w[c1[0]].shape, dw=g[c1[0]], dbias=g[c1[1]], ws=ws)
        dpool = ops.wide_conv2d_dgrad(dz, self._flip(c1[0]))
        # contracting path, from the bottom up
        dx = None
        for i in range(D - 2, -1, -1):
            c1, c2 = self.down[i]
            F = _filters(i, Fr)
            cat, a1, dcat = sv['cat'][i], sv['a1'][i], dcats[i]
            skip, dskip = cat[..., :F], dcat[..., :F]
            ops.pool2d_bwd(skip, dpool, p, 'max', dx=dskip, accumulate=True)
            dz = self._act_bwd_raw(dskip, skip, lid_of_block(i) + 1, ops.empty(skip.shape, skip.device))
            ops.wide_conv2d_wgrad(a1, dz, S.w[c2[0]].shape, dw=g[c2[0]], dbias=g[c2[1]], ws=ws)
            dz = ops.wide_conv2d_dgrad(dz, self._flip(c2[0]), act_out=a1, act=self.act, dropout=self._drop_of(lid_of_block(i)))
            pin = sv['pin'][i]
            ops.wide_conv2d_wgrad(pin, dz, S.w[c1[0]].shape, dw=g[c1[0]], dbias=g[c1[1]], ws=ws)
            if i > 0:
                dpool = ops.wide_conv2d_dgrad(dz, self._flip(c1[0]))
            elif need_dx:
                dx = ops.wide_conv2d_dgrad(dz, self._flip(c1[0]))
        self._saved = None
        if dx is None:
            return None
        return dx.reshape(N, 1, H, W) if self.in_channels == 1 else dx.permute(0, 3, 1, 2).contiguous()

    # ------------------------------------------------------------------ training (models/UNet.py:166-182)
    def _dummy_batch(self, shape):
        N, H, W = shape
        gen = torch.Generator(device='cpu').manual_seed(0)
        rhs = (torch.rand((N, self.in_channels, H, W), generator=gen) * 2 - 1).to(self.device)
        return (rhs, torch.full((N, 1), 0.02, device=self.device)), (torch.rand((N, self.out_channels, H, W), generator=gen) * 0.1).to(self.device)

    def _forward_backward(self, data):
        """pred = self(rhses) - no training=True, so the ConvBlocks' `if training:` dropout is off -, loss_fn(y, pred, rhs,
        concat([dx, dx], 1)) and its gradient into store.flat_g."""
        (rhs, dx), y_true = data
        rhs, dx, y_true = _as_device(rhs, self.device), _as_device(dx, self.device), _as_device(y_true, self.device)
        pred = self.call(rhs, training=False)
        loss, dpred = self.loss_fn.value_and_grad(y_true, pred, rhs, _dx_pair(_dx_column(dx)))
        self.backward(dpred, need_dx=False)
        return loss, y_true, pred

    def _eval_call(self, call_inputs):
        """evaluate / predict: the input list is [rhs, dx] as in the training data, the network takes the right-hand side alone."""
        return self.call(call_inputs[0], training=False)

    def grad_l2_norm(self):
        """'grad L2 norm' of UNetModel.train_step (:178): sqrt(mean over the trainable variables of sum(g^2)) - a device scalar."""
        sums = torch.stack([self.store.g[n].double().square().sum() for n in self.store.trainable_names()])
        return sums.mean().sqrt().float()

    def _extra_logs(self):
        return {'grad L2 norm': self.grad_l2_norm(), **super()._extra_logs()}


def UNet(nx=None, ny=None, in_channels=1, out_channels=1, layer_depth=5, filters_root=64, kernel_size=3, pool_size=2, dropout_rate=0.5,
         padding='valid', activation='relu', final_activation='linear', device=None, seed=0):
    """models/UNet.py:188-270 (same signature and defaults; `device` / `seed` are this library's)."""
    return UNetModel(nx=nx, ny=ny, in_channels=in_channels, out_channels=out_channels, layer_depth=layer_depth, filters_root=filters_root,
                     kernel_size=kernel_size, pool_size=pool_size, dropout_rate=dropout_rate, padding=padding, activation=activation,
                     final_activation=final_activation, device=device, seed=seed)
