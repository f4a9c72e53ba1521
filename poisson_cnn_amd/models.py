"""Homogeneous_Poisson_NN_Legacy on the libpcnn HIP kernels.

Drop-in for poisson_CNN/models/Homogeneous_Poisson_NN_Legacy.py:10-296: same constructor kwargs (the "model" section of
experiments/hpnn.json loads unchanged), `model([rhs, dx]) -> (N,1,H,W)`, `compile(loss, optimizer)`,
`train_step(((rhs, dx), y))`, `fit(sequence, epochs, callbacks)`, `trainable_variables`, `get_weights/set_weights`,
`save_weights/load_weights`, `summary()`.  The API is channels_first like the reference configs; inside, data is NHWC.
"""
import collections
import copy
import os

import numpy as np
import torch

from . import layers as L
from . import ops
from .utils import BC_EDGES, get_init_arguments_from_config, neumann_flags, neumann_mask, split_indices


def process_normalizations(normalizations):
    """models/Homogeneous_Poisson_NN_Metalearning.py:27-45."""
    types, defaults = ['rhs_max_magnitude'], [False]
    if normalizations is None:
        return dict(zip(types, defaults))
    normalizations = dict(normalizations)
    for k, d in zip(types, defaults):
        normalizations.setdefault(k, d)
    if isinstance(normalizations['rhs_max_magnitude'], bool) and normalizations['rhs_max_magnitude']:
        normalizations['rhs_max_magnitude'] = 1.0
    return normalizations


def process_output_scaling_modes(output_scalings):
    """models/Homogeneous_Poisson_NN_Metalearning.py:47-57."""
    modes = ['rhs_max_magnitude', 'max_domain_size_squared', 'match_peak_laplacian_magnitude_to_peak_rhs', 'soln_max_magnitude']
    out = {m: False for m in modes}
    if isinstance(output_scalings, dict):
        out.update(copy.deepcopy(output_scalings))
    return out


def _as_device(t, device):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.to(device=device, dtype=torch.float32).contiguous()


# what the constructors' "needs an AMD GPU" error adds about device="cpu" (_ModelBase._init_device)
_CPU_NOTE = ' (device="cpu" builds the parameter structure only)'
_CPU_NOTE_RAISES = ' (device="cpu" builds the parameter structure only; calling the model will raise)'


def _dx_column(dx):
    """A user's dx -> the (N,1) column the Legacy-family models work with: the first column of whatever width was given."""
    return dx.reshape(dx.shape[0], -1)[:, :1].contiguous()


def _dx_pair(dx):
    """That (N,1) column -> the (N,2) [dx, dx] which the loss and the Jacobi post-smoother take."""
    return torch.cat([dx, dx], 1)


def _dx_tiled(dx):
    """The _ChainModel / metalearning family's dx: one column is repeated for both axes (tf.tile(dx, [1, ndims])), two columns are kept."""
    dx = dx.reshape(dx.shape[0], -1)
    return dx.repeat(1, 2) if dx.shape[1] == 1 else dx


def _host_logs(logs):
    """train_step's dict with device scalars -> Python floats through ONE device-to-host copy (each float(tensor) is a stream synchronise of its own)."""
    dev = [(k, v) for k, v in logs.items() if isinstance(v, torch.Tensor)]
    out = {k: (v if isinstance(v, float) else float(v)) for k, v in logs.items() if not isinstance(v, torch.Tensor)}
    if dev:
        vals = torch.stack([v.reshape(()).float() for _, v in dev]).tolist()
        out.update({k: x for (k, _), x in zip(dev, vals)})
    return {k: out[k] for k in logs}


class _Prefetcher:
    """fit()'s input pipeline: batch i + 1 is produced while step i runs - what Keras' OrderedEnqueuer does for the reference's Sequence generators
    (train/hpnn_legacy_train.py:60 `model.fit(dataset, ...)`).  The generators of poisson_cnn_amd.dataset draw O(10)-sized parameters on the host
    (13 ms per batch of 50 for the shipped config) and synthesise the fields on the device: run on a stream of their own, their uploads and kernels
    do not queue behind the training step, and the host work hides under the step's kernels.  The consumer stream waits for the producer's event;
    the tensors are handed over with record_stream so that the caching allocator does not recycle them early.  PCNN_PREFETCH=0: generate in line."""

    def __init__(self, dataset, device):
        self.dataset = dataset
        self.on = os.environ.get('PCNN_PREFETCH', '1') != '0' and torch.cuda.is_available() and torch.device(device).type == 'cuda'
        self.stream = torch.cuda.Stream(device=device) if self.on else None
        self.pending = None

    def request(self, idx):
        if not self.on:
            self.pending = (idx, None, None)
            return
        # (no wait for the training stream: the generator allocates fresh tensors, and blocks the consumer released are recycled by the caching
        # allocator only after the events record_stream left on them - so the synthesis kernels overlap the step as well)
        with torch.cuda.stream(self.stream):
            batch = self.dataset[idx]
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.pending = (idx, batch, ev)

    def close(self):
        """Drops a batch that was requested and never taken, and the libpcnn handle of the producer stream (its scratch and workspaces)."""
        self.pending = None
        if self.on and self.stream is not None:
            try:
                self.stream.synchronize()
                ops.release_stream_handle(self.stream.cuda_stream, torch.device(self.stream.device).index)
            finally:
                self.stream = None
                self.on = False

    def take(self):
        idx, batch, ev = self.pending
        self.pending = None
        if ev is None:
            return self.dataset[idx]
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)

        def hand_over(v):
            if isinstance(v, torch.Tensor) and v.is_cuda:
                v.record_stream(cur)
            elif isinstance(v, (list, tuple)):
                for u in v:
                    hand_over(u)
        hand_over(batch)
        return batch


class _ModelBase:
    """What every model class shares: the Keras-style weight API over its ParamStore(s), compile(), presize(), the training step and fit().

    A model provides call(inp, training), backward(dpred) and ONE hook, _forward_backward(data) -> (loss, y_true, pred): channels-first data to the
    device, call, loss_fn.value_and_grad, backward - the gradient lands in every store's flat_g; no optimizer, no collective.  train_step is
    _local_step (that hook plus the mse metric: what graphs.GraphedTrainStep records) followed by _finish_step (gradient all-reduce, optimizer
    update, logs: the only place in the package that runs this sequence)."""
    model_name = 'model'

    def _init_device(self, device, cpu_note='', name=None):
        """The constructors' prologue: self.device (`device`, or the current GPU - there must be one) and the attributes compile() and
        parallel.DataParallel.attach fill in."""
        if device is None and not torch.cuda.is_available():
            raise RuntimeError('%s needs an AMD GPU: the HIP kernels are the only compute path%s' % (name or self.model_name, cpu_note))
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.optimizer = self.loss_fn = None
        self.grad_sync = None    # set by parallel.DataParallel: called with each store's flat gradient bucket before the optimizer step

    # ------------------------------------------------------------------ weights
    @property
    def trainable_variables(self):
        return [self.store.w[n] for n in self.store.trainable_names()]

    @property
    def weight_names(self):
        return self.store.names

    def get_weights(self):
        return [self.store.w[n].detach().cpu().numpy().copy() for n in self.store.names]

    def set_weights(self, weights):
        if isinstance(weights, dict):
            missing = set(self.store.names) - set(weights)
            if missing:
                raise ValueError('missing weights: %s' % sorted(missing)[:5])
            weights = [weights[n] for n in self.store.names]
        if len(weights) != len(self.store.names):
            raise ValueError('expected %d weight arrays, got %d' % (len(self.store.names), len(weights)))
        for n, v in zip(self.store.names, weights):
            v = np.asarray(v, dtype=np.float32)
            if tuple(v.shape) != tuple(self.store.w[n].shape):
                raise ValueError('shape mismatch for %s: %s vs %s' % (n, v.shape, tuple(self.store.w[n].shape)))
            self.store.w[n].copy_(torch.from_numpy(v))

    def save_weights(self, path, save_format=None):
        """Flat .npz keyed by parameter name (every model), or - save_format='tf' - the TensorFlow checkpoint pair <path>.index +
        <path>.data-00000-of-00001 that the reference's `model.save_weights(path)` writes (tf_checkpoint.py)."""
        if save_format in ('tf', 'tensorflow'):
            from .tf_checkpoint import save_tf_checkpoint
            return save_tf_checkpoint(self, str(path))
        if save_format not in (None, 'npz'):
            raise ValueError('save_format must be None / "npz" / "tf" (HDF5 is not supported)')
        np.savez(path, **{n.replace('/', '.'): w for n, w in zip(self.weight_names, self.get_weights())})

    def load_weights(self, path):
        path = str(path)
        if os.path.exists(path + '.index'):
            from .tf_checkpoint import load_tf_checkpoint
            return load_tf_checkpoint(self, path)
        with np.load(path if path.endswith('.npz') else path + '.npz') as z:
            self.set_weights({n: z[n.replace('/', '.')] for n in self.weight_names})

    def count_params(self):
        return self.store.n_trainable

    def summary(self, print_fn=print):
        print_fn('%s (MI355X / libpcnn)' % self.model_name)
        for name, shape, _, kind in self.store.specs:
            print_fn('  %-44s %-20s %s' % (name, shape, 'trainable' if kind in ('w', 'bn_gamma', 'bn_beta') else 'non-trainable'))
        print_fn('Trainable params: %d' % self.store.n_trainable)

    # ------------------------------------------------------------------ data_format
    # The network's boundary tensors all have ONE channel, so (N,1,H,W) and (N,H,W,1) are the same memory: data_format='channels_last' is a
    # reshape at the public entry points (__call__, train_step / fit); call() and everything inside stay channels_first.
    def _channels_last(self):
        return getattr(self, 'data_format', 'channels_first') == 'channels_last'

    def _cf(self, t):
        """one user tensor -> channels_first view: (N,H,W,1) -> (N,1,H,W), (N,L,1) -> (N,1,L); scalars / (N,k) arrays untouched"""
        if not self._channels_last() or not hasattr(t, 'shape') or len(t.shape) < 3:
            return t
        if t.shape[-1] != 1:
            raise ValueError('channels_last tensors of this model have one channel, got shape %s' % (tuple(t.shape),))
        t = torch.as_tensor(np.asarray(t)) if isinstance(t, np.ndarray) else t
        return t.reshape((t.shape[0], 1) + tuple(t.shape[1:-1]))

    def _cl(self, t):
        if not self._channels_last() or t.dim() < 3:
            return t
        return t.reshape((t.shape[0],) + tuple(t.shape[2:]) + (1,))

    def __call__(self, inp, training=False):
        return self._cl(self.call([self._cf(v) for v in inp], training=training))

    # ------------------------------------------------------------------ the training step
    def train_step(self, data):
        return self._finish_step(*self._local_step(data))

    def _local_step(self, data):
        """The part of a step that is a fixed launch sequence on this process: forward, loss, backward (the gradient in every store's flat_g) and
        the mse metric -> the device scalars (loss, mse) of the LOCAL batch."""
        inputs, y_true = data
        loss, y_true, pred = self._forward_backward(([self._cf(v) for v in inputs], self._cf(y_true)))
        return loss, self.loss_fn.mse_metric(y_true, pred)

    def _finish_step(self, loss, mse):
        """Gradient all-reduce (data parallel), the optimizer update, and the dict train_step returns."""
        if self.grad_sync is not None:
            for store in self.stores:
                self.grad_sync(store.flat_g)
        extra = self._extra_logs()
        self.optimizer.apply_gradients()
        return self._logs(loss, mse, extra)

    def _extra_logs(self):
        """Further train_step entries, computed on the synchronised gradient in front of the update (UNetModel: its gradient norm).  With a clip
        option of the optimizer set: 'grad_norm', the pre-clip global gradient norm - the optimizer's own device scalar, which the update that
        follows on the same stream fills before anything reads it."""
        opt = self.optimizer
        return {'grad_norm': opt.global_norm} if getattr(opt, 'clips', False) else {}

    @property
    def stores(self):
        return [self.store]

    def compile(self, loss, optimizer, max_input_shape=None):
        """max_input_shape = (per-process batch, H, W): the largest batch the training loop will see (train.main passes the maximum of the dataset's
        random_output_shape_range) - see presize()."""
        self.optimizer = optimizer
        self.loss_fn = loss
        optimizer.bind(self.stores)
        if max_input_shape is not None:
            self.presize(max_input_shape)

    def presize(self, max_input_shape):
        """One forward + backward on a synthetic batch of the LARGEST shape the training loop will see, without an optimizer step: the libpcnn handles'
        workspaces, the branch / side streams' scratch and torch's allocator pools all reach their high-water mark here, once.  The shipped training
        workload (experiments/hpnn.json:62-75: a new grid shape in [192, 384]^2 every batch, train/hpnn_legacy_train.py:26-60) otherwise re-grows them
        every time a larger shape comes along - a stream synchronise + free + allocate inside a convolution call, up to 0.6 s for one step
        (profiles/r06_train_shipped.txt).  Weights, optimizer state and BatchNormalization statistics are left exactly as they were."""
        batch = self._dummy_batch(tuple(int(v) for v in max_input_shape))
        if self.loss_fn is None:
            raise RuntimeError('presize() needs compile(loss, optimizer) first')
        stats = [(st, st.flat_stats.clone()) for st in self.stores if getattr(st, 'flat_stats', None) is not None]
        self._forward_backward(batch)
        for st in self.stores:
            st.flat_g.zero_()
        for st, snap in stats:
            st.flat_stats.copy_(snap)
        if getattr(self, '_acc', None) is not None:
            self._acc.zero_()
        torch.cuda.synchronize()

    def _dummy_batch(self, shape):
        raise NotImplementedError('%s: presize() needs a _dummy_batch(shape), which this model does not have' % type(self).__name__)

    metric_sync = None   # set by parallel.DataParallel.attach: (loss, mse) -> their GLOBAL values (one tiny all-reduce)

    def _logs(self, loss, mse, extra):
        """What train_step returns (`extra`: the model's own entries, placed before 'lr').
        Under data parallelism each rank's loss is its share of the global-batch loss (already divided by the global batch size, losses/loss_wrapper.py:46-49) and its mse the mean over its own samples; callbacks (ReduceLROnPlateau,
        TerminateOnNaN, ModelCheckpoint) must see the same GLOBAL numbers on every rank or the replicas' learning rates / stop decisions
        diverge - MirroredStrategy reduces the per-replica results the same way before Keras hands them to callbacks."""
        if self.metric_sync is not None:
            loss, mse = self.metric_sync(loss, mse)
        return {'loss': loss, 'mse': mse, **extra, 'lr': self.optimizer.learning_rate}

    # ------------------------------------------------------------------ evaluation: test_step / evaluate / predict
    eval_sync = None     # set by parallel.DataParallel.attach: (totals vector, maximum) of this rank -> of all ranks (global_eval_totals)

    @staticmethod
    def _loss_dx(dx):
        """The user's dx -> the (N,2) per-axis spacings this model's training step hands to the loss (and evaluation to ops.error_stats)."""
        return _dx_pair(_dx_column(dx))

    _call_takes_loss_dx = False

    def _eval_inputs(self, inputs, y_true):
        """A channels-first input list -> (what call() takes, rhs (N,1,H,W) or None, dx (N,2)).  The three input lists of the package:
        [rhs, dx] (homogeneous models, UNet), [bc, dx] / [bc, dx, x_output_resolution] (boundary models: no right-hand side, the resolution
        comes from the target when it is not given) and Poisson_CNN_Legacy's [rhs, left, top, right, bottom, dx]."""
        dev = self.device
        if len(inputs) == 6:
            rhs, dx = _as_device(inputs[0], dev), _as_device(inputs[5], dev)
            return [rhs] + list(inputs[1:5]) + [dx], rhs, self._loss_dx(dx).contiguous()
        if len(inputs) not in (2, 3):
            raise ValueError('%s: cannot evaluate an input list of %d entries' % (self.model_name, len(inputs)))
        first, dx = _as_device(inputs[0], dev), _as_device(inputs[1], dev)
        dx2 = self._loss_dx(dx).contiguous()
        if self._call_takes_loss_dx:                                 # the metalearning family's call() works on the per-axis spacings themselves
            dx = dx2
        if first.dim() == 4 and len(inputs) == 2:
            return [first, dx], first, dx2
        if len(inputs) == 2 and y_true is None:
            raise ValueError('%s: without a target the input list needs the x_output_resolution as its third entry' % self.model_name)
        return [first, dx, int(inputs[2]) if len(inputs) == 3 else int(y_true.shape[2])], None, dx2

    def _eval_call(self, call_inputs):
        return self.call(call_inputs, training=False)

    def _eval_forward(self, inputs, y_true=None):
        """The inference-mode forward of one batch of user tensors -> (pred, y_true, rhs, dx), channels-first on the device."""
        inputs = [self._cf(v) for v in inputs]
        if y_true is not None:
            y_true = _as_device(self._cf(y_true), self.device)
        call_inputs, rhs, dx = self._eval_inputs(inputs, y_true)
        return self._eval_call(call_inputs), y_true, rhs, dx

    @staticmethod
    def _error_stats(pred, y_true, rhs, dx):
        """ops.error_stats of a channels-first batch -> ((N, 8) rows, points per sample as (H, W)).  A model with several output channels
        (UNet(out_channels > 1)) gets the error columns over all its channels and no residual."""
        N, C, H, W = pred.shape
        if C != 1:
            return ops.error_stats(pred.reshape(N, C * H, W), None if y_true is None else y_true.reshape(N, C * H, W)), (C * H, W)
        if rhs is not None and (H < 3 or W < 3):
            rhs = None
        return ops.error_stats(pred, y_true, rhs, dx), (H, W)

    def test_step(self, data):
        """One batch (inputs, target) in inference mode: forward with training=False, the compiled loss and ops.error_stats - no backward pass, no
        optimizer step, no BatchNormalization update; weights, gradients, statistics and optimizer state keep their bits.  Returns device
        tensors: 'loss' (the compiled loss of this batch, i.e. divided by the loss's global_batch_size), 'mse', and 'stats', the (N, 8) rows of
        ops.error_stats (columns ops.ERROR_STATS; the residual columns are zero for a model without a right-hand side input)."""
        if self.loss_fn is None:
            raise RuntimeError('test_step() / evaluate() need compile(loss, optimizer) first')
        inputs, y_true = data
        pred, y_true, rhs, dx = self._eval_forward(inputs, y_true)
        loss_rhs = rhs
        if loss_rhs is None and getattr(self.loss_fn, 'physics_informed_loss_weight', 1.0) != 0.0:
            loss_rhs = torch.zeros_like(y_true)                      # the boundary models' training steps: the loss sees rhs = 0
        value = self.loss_fn.value if hasattr(self.loss_fn, 'value') else self.loss_fn
        loss = value(y_true, pred, loss_rhs, dx)
        stats, (H, W) = self._error_stats(pred, y_true, rhs, dx)
        return {'loss': loss, 'mse': stats[:, 1].sum() / float(stats.shape[0] * H * W), 'stats': stats, 'H': H, 'W': W}

    def _batches(self, x, y, batch_size, steps):
        from . import evaluation as E
        if E.is_sequence(x):
            if y is not None:
                raise ValueError('a Sequence-style dataset provides its own targets: y must be None')
            data = x
        else:
            data = E.ArrayBatches(x, y, batch_size)
        n = len(data)
        return data, (n if steps is None else min(int(steps), n))

    def evaluate(self, x=None, y=None, batch_size=None, steps=None, return_dict=False, per_sample=False, verbose=0, **unsupported):
        """Keras' Model.evaluate on the one-pass error kernel.  x: a Sequence-style dataset (`__len__`, `__getitem__` -> (inputs, target); the grid
        shape may change from batch to batch), or an input list with `y` the targets, cut into chunks of `batch_size` (default 32) samples.
        One host round trip per batch.  Over all evaluated samples:
          loss: mean per-sample compiled loss          mse, mae: sums over all points / number of points
          rel_l2: mean of sqrt(sum e^2 / sum t^2)      mae_over_peak: mean of (mean|e|) / max|t|          max_abs_error: maximum
          rel_residual: mean of sqrt(sum r^2 / sum f^2), r the 3 x 3 FD residual of the prediction, f the right-hand side
        Samples with a zero target (right-hand side) are left out of the relative means and counted under skipped_rel_l2
        (skipped_rel_residual).  A model without a right-hand side among its inputs (the Dirichlet boundary models) has no residual: rel_residual
        is NaN and every sample counts as skipped.  Returns [loss, mse], or the whole dict with return_dict=True; per_sample=True adds 'stats'
        (the (samples, 8) float64 rows of ops.error_stats) and 'H', 'W' per sample.  Under data parallelism every rank evaluates its own
        batches and the totals are combined (parallel.DataParallel.global_eval_totals), so all ranks return the same figures; 'stats' stays
        this rank's.  sample_weight and class_weight are not implemented."""
        from . import evaluation as E
        E.reject_unsupported('evaluate', unsupported)
        data, n = self._batches(x, y, batch_size, steps)
        totals, worst = np.zeros(len(E.TOTALS)), 0.0
        rows, hs, ws = [], [], []
        gbs = getattr(self.loss_fn, 'global_batch_size', None)
        fetch = _Prefetcher(data, self.device)
        try:
            if n > 0:
                fetch.request(0)
            for step in range(n):
                inp, tar = fetch.take()
                out = self.test_step((list(inp), tar))
                if step + 1 < n:
                    fetch.request(step + 1)
                flat = torch.cat([out['loss'].reshape(1).float(), out['stats'].reshape(-1)]).tolist()       # the batch's one host round trip
                stats = np.asarray(flat[1:], dtype=np.float64).reshape(-1, 8)
                t, m = E.batch_totals(stats, out['H'], out['W'], flat[0], gbs)
                totals += t
                worst = max(worst, m)
                if per_sample:
                    rows.append(stats)
                    hs += [out['H']] * stats.shape[0]
                    ws += [out['W']] * stats.shape[0]
                if verbose:
                    print('evaluate %d/%d - loss: %.6g' % (step + 1, n, flat[0] * (gbs or stats.shape[0]) / stats.shape[0]), flush=True)
        finally:
            fetch.close()
        if self.eval_sync is not None:
            totals, worst = self.eval_sync(totals, worst)
        res = E.finish(totals, worst)
        if per_sample:
            res.update(stats=np.concatenate(rows) if rows else np.zeros((0, 8)), H=np.asarray(hs, dtype=np.int64), W=np.asarray(ws, dtype=np.int64))
            return res
        return res if return_dict else [res['loss'], res['mse']]

    def predict(self, x, batch_size=None, steps=None, verbose=0, return_stats=False):
        """Keras' Model.predict.  x: an input list, cut into chunks of `batch_size` (default 32) samples, or a Sequence-style dataset whose
        targets - if it has any - are ignored (a boundary model then takes its x_output_resolution from the target's shape).  Returns ONE numpy
        array in the model's data_format when all batches share a grid shape, otherwise a LIST of per-batch arrays.  return_stats=True also
        returns the residual columns of ops.error_stats per sample - a (samples, 3) float64 array [sum r^2, max|r|, sum f^2] - which measure
        the solution's quality without a ground truth; it needs rhs and dx among the inputs.  Nothing in the model changes: no BatchNormalization
        update, no gradient, no optimizer state."""
        from . import evaluation as E
        if E.is_sequence(x):
            data = x
        else:
            data = E.ArrayBatches(x, None, batch_size)
        n = len(data) if steps is None else min(int(steps), len(data))
        preds, res = [], []
        for step in range(n):
            item = data[step]
            inp, tar = item if (isinstance(item, tuple) and len(item) == 2 and isinstance(item[0], (list, tuple))) else (item, None)
            pred, _, rhs, dx = self._eval_forward(list(inp), tar)
            if return_stats:
                if rhs is None:
                    raise ValueError('predict(return_stats=True) needs rhs and dx among the inputs')
                res.append(self._error_stats(pred, None, rhs, dx)[0][:, 5:])
            preds.append(self._cl(pred).cpu().numpy())
            if verbose:
                print('predict %d/%d' % (step + 1, n), flush=True)
        out = preds
        if preds and all(p.shape[1:] == preds[0].shape[1:] for p in preds):
            out = np.concatenate(preds, 0)
        if return_stats:
            return out, (torch.cat(res).cpu().numpy().astype(np.float64) if res else np.zeros((0, 3)))
        return out

    _VAL_KEYS = ('loss', 'mse', 'rel_l2', 'rel_residual')     # evaluate()'s entries that fit() reports as val_<key>

    def fit(self, dataset, epochs=1, callbacks=(), verbose=1, steps_per_epoch=None, validation_data=None, validation_steps=None, validation_freq=1,
            validation_batch_size=None, **unsupported):
        """Minimal Keras-style loop over a Sequence-like dataset (`__len__`, `__getitem__` -> ([rhs, dx], soln)).

        Keras semantics for a custom train_step that returns plain values (models/Homogeneous_Poisson_NN_Legacy.py:291): the dict handed
        to on_epoch_end / History is the LAST batch's (tf.keras Model.fit: `epoch_logs = copy.copy(logs)`), not an epoch average - so that
        is what ReduceLROnPlateau and ModelCheckpoint monitor here too.  The epoch means are added under `loss_epoch_mean` / `mse_epoch_mean`.
        Under data parallelism the values are global (see _logs), so every rank's callbacks decide alike.

        validation_data: a Sequence-style dataset or a tuple (inputs, targets).  After the training steps of every validation_freq-th epoch
        evaluate() runs on it (validation_steps batches; validation_batch_size for the tuple form) and val_loss, val_mse, val_rel_l2 and
        val_rel_residual join that epoch's logs - before the callbacks see them - and the history; an epoch without a validation run has
        none of them, as in Keras.  Without validation_data nothing changes.  validation_split, sample_weight and class_weight are not
        implemented."""
        from . import evaluation as E
        E.reject_unsupported('fit', unsupported)
        history = {'loss': [], 'mse': [], 'lr': [], 'loss_epoch_mean': [], 'mse_epoch_mean': []}
        validation = None
        if validation_data is not None:
            if int(validation_freq) < 1:
                raise ValueError('validation_freq must be >= 1')
            if E.is_sequence(validation_data):
                validation = dict(x=validation_data, steps=validation_steps)
            elif isinstance(validation_data, (tuple, list)) and len(validation_data) == 2:
                validation = dict(x=validation_data[0], y=validation_data[1], batch_size=validation_batch_size, steps=validation_steps)
            else:
                raise ValueError('validation_data must be a Sequence-style dataset or a tuple (inputs, targets)')
            validation['freq'] = int(validation_freq)
            history.update({'val_' + k: [] for k in self._VAL_KEYS})
        self.stop_training = False
        for cb in callbacks:
            cb.set_model(self)
        fetch = _Prefetcher(dataset, self.device)             # one producer stream (and one libpcnn handle on it) per fit() call
        try:
            return self._fit_epochs(dataset, epochs, callbacks, verbose, steps_per_epoch, history, fetch, validation)
        finally:
            fetch.close()

    def _fit_epochs(self, dataset, epochs, callbacks, verbose, steps_per_epoch, history, fetch, validation=None):
        for epoch in range(epochs):
            n = steps_per_epoch if steps_per_epoch is not None else len(dataset)
            agg = {'loss': 0.0, 'mse': 0.0}
            logs = {'loss': float('nan'), 'mse': float('nan')}
            step = -1
            if n > 0:
                fetch.request(0)
            for step in range(n):
                inp, tar = fetch.take()
                logs = self.train_step((tuple(inp), tar))
                if step + 1 < n:                               # the next batch is generated (host draws + uploads + synthesis kernels on a stream of its
                    fetch.request(step + 1)                    # own) while this step's kernels run; dataset[step] is still called once per step, in order
                logs = _host_logs(logs)                        # the step's one host round trip
                for k in agg:
                    agg[k] += logs[k]
                for cb in callbacks:
                    cb.on_batch_end(step, logs)
                if self.stop_training:
                    break
            logs = {'loss': logs['loss'], 'mse': logs['mse'], 'lr': self.optimizer.learning_rate,
                    'loss_epoch_mean': agg['loss'] / max(step + 1, 1), 'mse_epoch_mean': agg['mse'] / max(step + 1, 1)}
            val_line = ''
            if validation is not None and (epoch + 1) % validation['freq'] == 0:
                res = self.evaluate(return_dict=True, **{k: v for k, v in validation.items() if k != 'freq'})
                logs.update({'val_' + k: res[k] for k in self._VAL_KEYS})
                val_line = ''.join(' - val_%s: %.6g' % (k, res[k]) for k in self._VAL_KEYS)
            for k in logs:
                history[k].append(logs[k])
            if verbose:
                print('Epoch %d/%d - loss: %.6g - mse: %.6g - lr: %.3g (epoch mean loss %.6g)%s'
                      % (epoch + 1, epochs, logs['loss'], logs['mse'], logs['lr'], logs['loss_epoch_mean'], val_line), flush=True)
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
            if hasattr(dataset, 'on_epoch_end'):
                dataset.on_epoch_end()
            if self.stop_training:
                break
        return history


_BRANCH_STREAMS = os.environ.get('PCNN_BRANCH_STREAMS', '1') != '0'      # 0: the coarse bottleneck branches stay on the main stream

MergePlan = collections.namedtuple('MergePlan', 'pyramid order stream tail')


def merge_plan(branches, H, W, coarse_factor):
    """What the bottleneck merge does on an H x W grid - host arithmetic only, no tensor and no stream.  branches: one (factor, 'pool' | 'conv'
    down-sampling, pool kind, resize method or None) per branch, in the model's order.  Returns
      pyramid  {factor: parent factor or None}, in the order the levels are pooled.  The branches average-pool the SAME tensor by 2, 3, 4, 8, ...
               (blocks/bottleneck_block.py:36-41): one full-resolution read each.  Where a factor f and an already pooled factor g | f both divide
               the image (no SAME padding), pool_f = pool_{f/g} o pool_g exactly (equal-weight means of equal-size blocks), so only the factors
               without a divisor read the full tensor.  A branch whose factor is a level takes that level as its input.
      order    the branch indices in the order they accumulate into the merge buffer: the coarse ones (factor >= coarse_factor) last
      stream   {coarse branch index: stream index}.  A branch that pools the full-resolution tensor itself (its factor does not divide the image)
               accumulates its input gradient into d_initial in the backward pass: all such branches share stream 0, so that they do so one after
               the other; every pyramid-fed one has a stream of its own
      tail     the resize branches at the end of `order` that one ops.resize_fwd_multi pass sums: at most three, never the whole order, ended by
               a branch without a resize method; fewer than two: none"""
    pyramid = {}
    for f in sorted({f for f, down, pool, _ in branches if down == 'pool' and pool in ('average', 'avg') and H % f == 0 and W % f == 0}):
        pyramid[f] = max([g for g in pyramid if f % g == 0], default=None)
    coarse = [i for i, b in enumerate(branches) if b[0] >= coarse_factor]
    order = [i for i in range(len(branches)) if i not in coarse] + coarse
    stream = {i: (k + 1 if branches[i][0] in pyramid else 0) for k, i in enumerate(coarse)}
    ntail = 0
    while ntail < min(3, len(order) - 1) and branches[order[-1 - ntail]][3] is not None:
        ntail += 1
    return MergePlan(pyramid, order, stream, order[len(order) - ntail:] if ntail >= 2 else [])


class _BottleneckMerge:
    """The merge stage of Homogeneous_Poisson_NN_Legacy (reference :204-222): every bottleneck branch reads `initial`, and their up-sampled outputs
    are summed, scaled by 1 / (branches x filters), into the merge buffer.  forward() / backward() execute merge_plan(); between them this object
    keeps `initial`, the pooling pyramid and the stream each branch ran on."""

    def __init__(self, blocks, ctx, filters):
        self.blocks, self.ctx = list(blocks), ctx
        self.branches = [(b.f, b.down_method, b.pool, b.resize_method) for b in self.blocks]
        self.alpha = 1.0 / float(len(self.blocks) * filters)     # :222
        self._saved = None

    def pool_pyramid(self, x, plan):
        """{factor: pooled x} of plan.pyramid, each level pooled from its parent."""
        pyr = {}
        for f, parent in plan.pyramid.items():
            pyr[f] = ops.pool2d_fwd(x if parent is None else pyr[parent], f if parent is None else f // parent, 'average')
        return pyr

    def forward(self, initial, merged, training, coarse_factor):
        """merged (a channel slice of the concatenation buffer) = alpha * sum over the branches of up(convs(down(initial)))."""
        H, W = initial.shape[1], initial.shape[2]
        blocks, alpha = self.blocks, self.alpha
        plan = merge_plan(self.branches, H, W, coarse_factor)
        pyr = self.pool_pyramid(initial, plan)
        # The eight branches are independent between the pooling pyramid and the merge buffer, and the coarse ones (factor >= 8: images of 128^2 and
        # below at 1024^2) are chains of launches that fill a fraction of the chip - 7.9 ms per training step back to back (tools/probe_branches.py).
        # Their convolution stages run on streams of their own (each stream has its libpcnn handle and its scratch, layers.Context), so that one
        # branch's small or tailing launches fill the gaps of another's; only the up-sampling, which accumulates into the shared merge buffer, stays on
        # the main stream.  The accumulation order is the same with and without the streams, so the result does not depend on the mode.
        pending, streams = {}, {}
        if plan.stream and self.ctx.use_side and _BRANCH_STREAMS:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            for i, k in plan.stream.items():
                st = self.ctx.branch_stream(k)
                with torch.cuda.stream(st):
                    st.wait_event(ready)
                    o = blocks[i].forward_convs(initial, training, pyr.get(blocks[i].f))
                    done = torch.cuda.Event()
                    done.record(st)
                pending[i] = (o, done)
                if training:
                    streams[i] = st
        # The eight branches accumulate into the merge slice (8 x 1024^2 x 32 channels: 1.07 GB, read and written once per branch); the resize branches at the end of
        # the order are summed in ONE read-modify-write pass (ops.resize_fwd_multi: the arithmetic and order of their separate calls, bit for bit).  (Measured and
        # rejected, round 6: running the accumulation over batch chunks of <= 160 MB of merge slice, every branch per chunk, so that a chunk would stay in the 256 MB
        # Infinity Cache between its passes - the single-stream step did not move, 195.4 vs 195.2 ms.)
        tail = []
        for n, i in enumerate(plan.order):
            b = blocks[i]
            if i in pending:                                          # (a branch is waited for right before ITS up-sampling: the later branches' convolution
                o, done = pending[i]                                  # stages keep running on their streams under the earlier branches' up-sampling)
                torch.cuda.current_stream().wait_event(done)
                o.record_stream(torch.cuda.current_stream())
            else:
                o = b.forward_convs(initial, training, pyr.get(b.f))
            b.note_upsampled(o, training)
            if i in plan.tail:
                tail.append((b, o))
            else:
                b.up_into(o, (H, W), merged, alpha, 0.0 if n == 0 else 1.0)
        if tail and ops.resize_fwd_multi([o for _, o in tail], (H, W), [b.resize_method for b, _ in tail], alpha=alpha, beta=1.0, out=merged) is None:
            for b, o in tail:
                b.up_into(o, (H, W), merged, alpha, 1.0)
        self._saved = (initial, pyr, plan.pyramid, streams) if training else None

    def backward(self, dmerged, d_initial):
        """Adds the merge stage's gradient with respect to `initial` into d_initial (and fills the branches' weight gradients)."""
        initial, pyr, parents, streams = self._saved
        self._saved = None
        alpha = self.alpha
        grads = {}
        late = []
        main = torch.cuda.current_stream()

        def add(f, g):
            grads[f] = g if f not in grads else ops.axpby(1.0, g, 1.0, grads[f])
        for i, b in enumerate(self.blocks):
            st = streams.get(i)
            if st is None:
                # a branch that pools the full-resolution tensor itself ADDS into d_initial: on the main stream that must come after every
                # stream-run branch that did the same (they share stream 0 among themselves; ADVICE r4: non-default PCNN_COARSE_FACTOR / factor orders)
                for _, g_prev, done_prev in late:
                    if g_prev is None:
                        main.wait_event(done_prev)
                g = b.backward_from(dmerged, alpha, d_initial)
                if g is not None:
                    add(b.f, g)
                continue
            dco = b.backward_up(dmerged, alpha)                       # reads the shared gradient: main stream
            ev = torch.cuda.Event()
            ev.record(main)
            with torch.cuda.stream(st):                               # the branch's convolution stages: the stream its saved activations live on
                st.wait_event(ev)
                dco.record_stream(st)
                g = b.backward_convs(dco, d_initial)                 # pyramid-fed: returns the pooled gradient; else adds into d_initial (stream 0 only)
                done = torch.cuda.Event()
                done.record(st)
            late.append((b, g, done))
        for b, g, done in late:
            main.wait_event(done)
            if g is not None:
                g.record_stream(main)
                add(b.f, g)
        for f in sorted(grads, reverse=True):                      # the pyramid's adjoint: coarsest level first, each into its parent
            parent = parents[f]
            if parent is None:
                ops.pool2d_bwd(initial, grads[f], f, 'average', dx=d_initial, accumulate=True)
            else:
                if parent not in grads:
                    grads[parent] = torch.zeros_like(pyr[parent])
                ops.pool2d_bwd(pyr[parent], grads[f], f // parent, 'average', dx=grads[parent], accumulate=True)


class Homogeneous_Poisson_NN_Legacy(_ModelBase):
    model_name = 'Homogeneous_Poisson_NN_Legacy'

    def __init__(self, data_format='channels_first', final_convolutions_config=None, pre_bottleneck_convolutions_config=None,
                 bottleneck_deconv_config=None, bottleneck_multilinear_config=None, input_normalization=None, output_scaling=None,
                 use_batchnorm=False, postsmoother_iterations=5, use_scaling=False, use_positional_embeddings=True, scaling_config=None,
                 gradient_accumulation_steps=None, bc_type='dirichlet', device=None, seed=0, batchnorm_training=False, smoother_boundaries='frozen',
                 density_input=False, boundary_types=None, residual_metrics=False):
        """bc_type: 'dirichlet' or 'neumann' for all four edges (the reference), or - an extension - a dict 'left' | 'right' | 'bottom' | 'top' ->
        'dirichlet' | 'neumann' with the dataset's edge names (left: y = 0, right: y = H-1, bottom: x = 0, top: x = W-1 of the (N,1,H,W) output; a missing
        edge is Dirichlet, at a corner a Dirichlet edge wins).  A Neumann edge is enforced as the reference's SYMMETRIC ring does, to first order:
        u_0 = u_1.
        smoother_boundaries: 'frozen' - the post-smoother keeps the ring it is given, as the reference's does, so its sweeps move the interior away
        from a Neumann edge's mirror values; 'enforce' - the smoother re-imposes the model's Neumann edges after every sweep
        (layers.JacobiIterationLayer(boundary_types=...)); with no Neumann edge there is nothing to enforce and the two are the same.
        density_input (extension): the model of the variable-density problem div((1/rho) grad u) = f.  call takes
        [stack (N,2,H,W), dx] with the stack [rhs, rho] of dataset.variable_density_dataset_generator; the first convolution sees [rhs, rho] and then
        the positional channels; Scaling reads the rhs channel; the post-smoother is layers.VariableDensityJacobiLayer; the loss to compile is
        losses.variable_density_loss_wrapper.  bc_type stays 'dirichlet' (it is the constant-coefficient model's switch and means the first-order
        SYMMETRIC ring); Neumann edges of the variable-density problem come in under boundary_types.  evaluate() / predict(return_stats=True) report the error
        statistics; the residual columns of ops.error_stats are the constant-coefficient residual and are left at 0 for such a model.
        boundary_types (density_input=True only): None, or a dict edge -> 'dirichlet' | 'neumann' as the variable-density solver
        and generator take it (a missing edge is Dirichlet).  The nodes of a Neumann edge are unknowns with du/dn = 0 in the solver's half-cell
        closure.  The ring is ops.bc_ring_fwd with that mask: Dirichlet edges become 0, a Neumann edge takes the mirror value, which is the
        smoother's starting value there; the post-smoother is layers.VariableDensityJacobiLayer(boundary_types=...), whose sweeps then move the
        Neumann edges' nodes by that closure.  Compile losses.variable_density_loss_wrapper with the same boundary_types.  All four edges Neumann
        is allowed and the model removes no mean: the residual term is blind to constants, the supervised terms (MAE, MSE, integral) pin the
        mean to the target's - the generator's solutions have zero w-mean.
        residual_metrics (density_input=True only; default False: nothing above changes): True fills the residual columns
        of the statistics with the flux-form figures of ops.varcoef_error_stats(neumann_mask=the model's) - sum w r^2, max|r|, sum w f^2 over the
        unknowns, du/dn = 0 on a Neumann edge - so test_step, evaluate, predict(return_stats=True) and fit(validation_data=...) report
        rel_residual = mean of sqrt(sum w r^2 / sum w f^2), the prediction_relative_residual of solve(), and callbacks can monitor
        val_rel_residual; solve(return_info=True) then returns prediction_max_residual with Neumann edges too.  It adds no variable: a
        checkpoint holds no trace of it."""
        if data_format not in ('channels_first', 'channels_last'):
            raise ValueError('data_format must be channels_first or channels_last')
        if pre_bottleneck_convolutions_config is None:
            raise ValueError('Provide a config for pre bottleneck convolutions')
        if bottleneck_deconv_config is None or bottleneck_multilinear_config is None:
            raise ValueError('Provide a config for bottleneck blocks')
        if final_convolutions_config is None:
            raise ValueError('Provide a config for final convolutions')
        if bc_type is None:
            raise ValueError('bc_type can only be neumann or dirichlet.')
        flags = neumann_flags(bc_type)
        if smoother_boundaries not in ('frozen', 'enforce'):
            raise ValueError("smoother_boundaries can only be 'frozen' or 'enforce'.")
        self.density_input = bool(density_input)
        if self.density_input and (isinstance(bc_type, dict) or any(flags)):
            raise NotImplementedError('density_input=True needs bc_type "dirichlet": the variable-density solver, loss and smoother have Dirichlet edges '
                                      'only (got bc_type %r)' % (bc_type,))
        if boundary_types is not None:
            if not self.density_input:
                raise ValueError('boundary_types is the keyword of the variable-density model (density_input=True); the constant-coefficient '
                                 "model takes its boundary types as bc_type ('dirichlet', 'neumann' or a dict per edge), got boundary_types %r" % (boundary_types,))
            if not isinstance(boundary_types, dict):
                raise ValueError("boundary_types is None or a dict edge -> 'dirichlet' | 'neumann', got %r" % (boundary_types,))
            flags = neumann_flags(boundary_types)                 # refuses an unknown edge name or type
        self.boundary_types = None if boundary_types is None else {e: 'neumann' if f else 'dirichlet' for e, f in zip(BC_EDGES, flags)}
        if residual_metrics and not self.density_input:
            raise ValueError('residual_metrics=True reports the flux-form residual of the variable-density model and needs density_input=True; the '
                             'constant-coefficient model always reports its 3 x 3 residual')
        self.residual_metrics = bool(residual_metrics)
        if self.density_input and data_format != 'channels_first':
            raise NotImplementedError('density_input=True: the two-channel stack is channels_first (N,2,H,W) only')
        self._init_device(device, _CPU_NOTE_RAISES)
        self.ndims = 2
        self.data_format = data_format
        self.gradient_accumulation_steps = gradient_accumulation_steps
        self.input_normalization = process_normalizations(input_normalization)
        self.output_scaling = process_output_scaling_modes(output_scaling)
        self.use_batchnorm = use_batchnorm
        self.use_positional_embeddings = use_positional_embeddings
        self.neumann_mask = neumann_mask(bc_type if boundary_types is None else boundary_types)   # the model's one record of its boundary types (bits as ops.bc_ring_fwd's)
        self.per_edge_bc = isinstance(bc_type, dict)              # how bc_type was given; a uniform dict and the string run the same kernels
        self.store = S = L.ParamStore()
        # BatchNormalization mode inside train_step: False = moving statistics (what the reference's train_step most likely does,
        # SURVEY.md row H4), True = batch statistics + moving-average update (Keras training=True semantics, per replica)
        S.bn_training = bool(batchnorm_training)
        self.ctx = C = L.Context()
        C.enable_side_stream()

        # pre-bottleneck convolutions (reference :41-57)
        pre = copy.deepcopy(pre_bottleneck_convolutions_config)
        mode, val = pre.pop('padding_mode', 'CONSTANT'), pre.pop('constant_padding_value', 0.0)
        self.pre = []
        cin = (2 if self.density_input else 1) + (2 if use_positional_embeddings else 0)
        for k in range(len(pre['filters'])):
            a = get_init_arguments_from_config(pre, k, ['filters', 'kernel_sizes'], ['filters', 'kernel_size'])
            self.pre.append(L.ConvUnit(S, C, 'pre/conv%d' % k, a['kernel_size'], cin, a['filters'], padding_mode=mode, pad_value=val,
                                       activation=a.get('activation', 'linear'), use_bias=a.get('use_bias', True),
                                       bn_name=('pre/bn%d' % k) if use_batchnorm else None))
            cin = a['filters']
        c0 = cin
        # bottleneck blocks (:59-69), sorted by descending downsampling factor
        assert bottleneck_deconv_config['filters'] == bottleneck_multilinear_config['filters']
        F = self.filters = bottleneck_deconv_config['filters']
        dfields = ['downsampling_factors', 'upsampling_factors', 'conv_kernel_sizes', 'deconv_kernel_sizes', 'n_convs']
        dargs = ['downsampling_factor', 'upsampling_factor', 'conv_kernel_size', 'deconv_kernel_size', 'n_convs']
        dcfgs = [get_init_arguments_from_config(bottleneck_deconv_config, k, dfields, dargs) for k in range(len(bottleneck_deconv_config['downsampling_factors']))]
        dcfgs = sorted(dcfgs, key=lambda a: a['downsampling_factor'], reverse=True)
        self.bottleneck_deconv_blocks = [L.bottleneck_block_deconvupsample(S, C, 'deconv_f%d' % a['downsampling_factor'], c0, use_batchnorm=use_batchnorm, **a)
                                         for a in dcfgs]
        mfields = ['downsampling_factors', 'upsampling_factors', 'conv_kernel_sizes', 'n_convs'] + (['resize_methods'] if 'resize_methods' in bottleneck_multilinear_config else [])
        margs = ['downsampling_factor', 'upsampling_factor', 'conv_kernel_size', 'n_convs'] + (['resize_method'] if 'resize_methods' in bottleneck_multilinear_config else [])
        mcfgs = [get_init_arguments_from_config(bottleneck_multilinear_config, k, mfields, margs) for k in range(len(bottleneck_multilinear_config['downsampling_factors']))]
        mcfgs = sorted(mcfgs, key=lambda a: a['downsampling_factor'], reverse=True)
        self.bottleneck_multilinear_blocks = [L.bottleneck_block_multilinearupsample(S, C, 'multilinear_f%d' % a['downsampling_factor'], c0, use_batchnorm=use_batchnorm, **a)
                                              for a in mcfgs]
        # merge + post-merge (:71-76)
        self.merge = _BottleneckMerge(self.bottleneck_deconv_blocks + self.bottleneck_multilinear_blocks, C, F)
        self.non_bottleneck_conv = L.ConvUnit(S, C, 'non_bottleneck_conv', 5, c0, F, pad='same', activation='leaky_relu')
        self.post_merge_conv = L.ConvUnit(S, C, 'post_merge_conv', 7, 2 * F, F, pad='same', activation='leaky_relu')
        self.post_merge_resnet = L.resnet(S, C, 'post_merge_resnet', F, 7, activation='leaky_relu')
        # final convolutions (:78-96)
        fc = copy.deepcopy(final_convolutions_config)
        nst = len(fc['filters'])
        fmode, fval = fc.pop('padding_mode', 'CONSTANT'), fc.pop('constant_padding_value', 0.0)
        nreg = fc.pop('final_regular_conv_stages', 2)
        self.final = []
        cin = F
        for k in range(nst - nreg):
            a = get_init_arguments_from_config(fc, k, ['filters', 'kernel_sizes'], ['filters', 'kernel_size'])
            act, ub = a.get('activation', 'linear'), a.get('use_bias', True)
            self.final.append(L.ConvUnit(S, C, 'final/stage%d/conv' % k, a['kernel_size'], cin, a['filters'], padding_mode=fmode, pad_value=fval,
                                         activation=act, use_bias=ub))
            self.final.append(L.resnet(S, C, 'final/stage%d/res' % k, a['filters'], a['kernel_size'], padding_mode='constant', activation=act, use_bias=ub))
            cin = a['filters']
        for j, k in enumerate(range(nst - nreg, nst)):
            self.final.append(L.ConvUnit(S, C, 'final/out%d' % j, fc['kernel_sizes'][k], cin, fc['filters'][k], pad='same', activation='linear',
                                         use_bias=fc.get('use_bias', True)))
            cin = fc['filters'][k]
        if cin != 1:
            raise ValueError('the last final convolution must have 1 filter')
        # dx dense layers (:98-102)
        units = [100, 100, F]
        acts = ['leaky_relu', 'leaky_relu', 'linear']
        self.dx_dense_layers = []
        din = 3
        for i, (u, a) in enumerate(zip(units, acts)):
            self.dx_dense_layers.append(L.Dense(S, 'dx_dense%d' % i, din, u, a))
            din = u
        enforce = None
        if smoother_boundaries == 'enforce' and self.neumann_mask:
            enforce = {e: 'neumann' if f else 'dirichlet' for e, f in zip(BC_EDGES, flags)}
        if self.density_input:
            self.postsmoother = L.VariableDensityJacobiLayer(postsmoother_iterations, boundary_types=self.boundary_types) if postsmoother_iterations > 0 else None
        else:
            self.postsmoother = L.JacobiIterationLayer(postsmoother_iterations, boundary_types=enforce) if postsmoother_iterations > 0 else None
        self.scaling = L.Scaling(S, C, 'scaling', **scaling_config) if use_scaling else None
        S.finalize(self.device)
        S.initialize(seed)
        self._acc = None

    COARSE_FACTOR = int(os.environ.get('PCNN_COARSE_FACTOR', '2'))     # bottleneck branches from this down-sampling factor on (default: all of them) run their
                                                                        # convolution stages on streams of their own; measured at 8 x 1024^2: none 243, >= 8: 238.9, all: 236 ms per step

    # ------------------------------------------------------------------ forward
    def _assemble(self, rhs):
        """The network's NHWC input and the one-channel (N,H,W) fields Scaling and the smoother read: (x, rhs_hw, rho_hw - None without density_input)."""
        if self.density_input:
            if rhs.dim() != 4 or rhs.shape[1] != 2:
                raise ValueError('a density_input model takes the stack [rhs, rho] of shape (N,2,H,W)')
            stack = rhs.contiguous()
            rhs_hw, rho_hw = stack[:, 0].contiguous(), stack[:, 1].contiguous()
            return ops.assemble_density_input(stack, self.use_positional_embeddings), rhs_hw, rho_hw
        if rhs.dim() != 4 or rhs.shape[1] != 1:
            raise ValueError('rhs must have shape (N,1,H,W)')
        rhs_hw = rhs.view(rhs.shape[0], rhs.shape[2], rhs.shape[3])
        return ops.assemble_input(rhs_hw, self.use_positional_embeddings), rhs_hw, None

    def _smooth(self, x, rhs_hw, rho_hw, dx, training):
        """The post-smoother on the prediction x (N,H,W,1): the flux-form sweeps when there is a density field, else the constant-coefficient ones."""
        if self.postsmoother is None:
            return x
        rhs = rhs_hw.unsqueeze(-1)
        if rho_hw is not None:
            return self.postsmoother.forward(x, rhs, rho_hw.unsqueeze(-1), dx, training=training)
        return self.postsmoother.forward(x, rhs, _dx_pair(dx), training=training)

    def call(self, inp, training=False):
        """reference :183-257.  inp = [rhs (N,1,H,W), dx (N,1)]; returns (N,1,H,W) (torch CUDA tensor).  density_input: inp = [stack (N,2,H,W), dx],
        the stack [rhs, rho]."""
        rhs, dx = inp
        rhs = _as_device(rhs, self.device)
        dx = _as_device(dx, self.device)
        x, rhs_hw, rho_hw = self._assemble(rhs)                 # refuses a malformed rhs before anything else is looked at or done
        dx = self._spacing_column(dx)
        N, H, W = rhs_hw.shape
        S = self.store
        S.refresh_bn()
        # dense input [dx, Lx, Ly] (:193,:202): tiny (N,3) host-side assembly
        dense_inp = torch.cat([dx, dx * float(H - 1), dx * float(W - 1)], 1).contiguous()
        hint = None                                               # max|x| travels with the tensor from layer to layer (weight-gradient scaling)
        for c in self.pre:
            x = c.forward(x, training=training, x_absmax=hint)
            hint = c.out_absmax
        initial = x
        F = self.filters
        cat = ops.empty((N, H, W, 2 * F), self.device)       # [non_bottleneck_conv | merged] (tf.concat axis=1, :224)
        self.merge.forward(initial, cat[..., F:], training, self.COARSE_FACTOR)     # the bottleneck branches, summed (:204-222)
        self.non_bottleneck_conv.forward(initial, out=cat[..., :F], training=training)
        x = self.post_merge_conv.forward(cat, training=training)
        x = self.post_merge_resnet.forward(x, training=training, x_absmax=self.post_merge_conv.out_absmax)
        d = dense_inp
        for lyr in self.dx_dense_layers:
            d = lyr.forward(d, training=training)
        xs = ops.channel_scale_fwd(x, d)                          # :231
        if training:
            self._saved = {'scale_in': x, 'dx_info': d, 'shape': (N, H, W)}
        x = xs
        hint = None
        for lyr in self.final:
            x = lyr.forward(x, training=training, x_absmax=hint)
            hint = lyr.out_absmax
        if self.scaling is not None:
            x = self.scaling.forward(x, rhs_hw.view(N, H, W, 1), training=training)
        x = ops.bc_ring_fwd(x, self.neumann_mask)               # :251
        return self._smooth(x, rhs_hw, rho_hw, dx, training).view(N, 1, H, W)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred):
        """Back-propagates dL/dpred (N,1,H,W) through the graph saved by call(training=True); fills store.flat_g."""
        sv = self._saved
        self._saved = None
        N, H, W = sv['shape']
        F = self.filters
        d = dpred.contiguous().view(N, H, W, 1)
        if self.postsmoother is not None:
            d = self.postsmoother.backward(d)
        d = ops.bc_ring_bwd(d, self.neumann_mask)
        if self.scaling is not None:
            d = self.scaling.backward(d)
        ready = False                                              # the gradient arriving at a layer already went through its activation backward
        for i in reversed(range(len(self.final))):                 # (fused into the data-gradient kernel of the layer after it, layers.ConvUnit.post_spec)
            post = self.final[i - 1].post_spec() if i > 0 else None
            d = self.final[i].backward(d, inplace=True, dz_ready=ready, post=post)
            ready = post is not None and post.applied
        # the einsum's input is post_merge_resnet's activation output: its adjoint also applies that layer's activation backward (one pass of a full-
        # resolution 32-channel tensor instead of four; ops.channel_scale_bwd_post declines where the offer does not fit)
        ps = self.post_merge_resnet.post_spec()
        fused = ops.channel_scale_bwd_post(sv['scale_in'], sv['dx_info'], d, ps, ws=self.ctx.ws)
        if fused is not None:
            d, ds = fused
        else:
            d, ds = ops.channel_scale_bwd(sv['scale_in'], sv['dx_info'], d, ws=self.ctx.ws)
        dd = ds
        for i, lyr in enumerate(reversed(self.dx_dense_layers)):
            dd = lyr.backward(dd, need_dx=(i < len(self.dx_dense_layers) - 1))
        post = self.post_merge_conv.post_spec()
        d = self.post_merge_resnet.backward(d, inplace=True, dz_ready=fused is not None, post=post)
        dcat = self.post_merge_conv.backward(d, inplace=True, dz_ready=post is not None and post.applied)
        d_initial = self.non_bottleneck_conv.backward(dcat[..., :F], inplace=False)
        self.merge.backward(dcat[..., F:], d_initial)
        d = d_initial
        for i, c in enumerate(reversed(self.pre)):
            d = c.backward(d, need_dx=(i < len(self.pre) - 1), inplace=True)
        self.ctx.join()                                            # weight gradients of the side stream
        self.store.finish_bn_grads()

    # ------------------------------------------------------------------ training (reference :259-296)
    def _loss_and_grads(self, rhs, dx, y_true):
        pred = self.call([rhs, dx], training=True)
        loss, dpred = self.loss_fn.value_and_grad(y_true, pred, rhs, dx if self.density_input else _dx_pair(dx))   # (one spacing per sample: no column check)
        self.backward(dpred)
        return loss, pred

    def _spacing_column(self, dx):
        """_dx_column; a density_input model refuses columns that differ (the first one alone would be used, and the loss would never see the other)."""
        if self.density_input:
            cols = dx.reshape(dx.shape[0], -1)
            if cols.shape[1] > 1 and not bool((cols == cols[:, :1]).all()):
                raise NotImplementedError('density_input=True: anisotropic spacing (dx columns that differ) is not supported - pass one spacing per '
                                          'sample, dx of shape (N,1)')
        return _dx_column(dx)

    def _error_stats(self, pred, y_true, rhs, dx):
        """density_input: `rhs` is the [rhs, rho] stack and the residual columns of ops.error_stats are the constant-coefficient residual - they stay 0,
        unless residual_metrics asks for the flux-form ones (ops.varcoef_error_stats with the model's mask)."""
        if not self.residual_metrics:
            return _ModelBase._error_stats(pred, y_true, None if self.density_input else rhs, dx)
        N, _, H, W = pred.shape
        if H < 3 or W < 3:
            return ops.varcoef_error_stats(pred, None, y_true), (H, W)
        return ops.varcoef_error_stats(pred, rhs[:, 1].contiguous(), y_true, rhs[:, 0].contiguous(), _dx_column(dx), neumann_mask=self.neumann_mask), (H, W)

    def solve(self, inputs, tol=1e-10, max_iterations=500, check_every=8, warm_start=True, compare_cold=False, return_info=False, preconditioner='dst'):
        """The variable-density problem solved to `tol`, the conjugate-gradient iteration started from this model's prediction (DESIGN.md section
        18).  inputs = [stack (N,2,H,W) = [rhs, rho], dx] as for call; the edges are zero, as the model's are.  Runs the inference-mode forward,
        ops.varcoef_error_stats on the prediction, and dataset.variable_density_poisson_solve(rho, rhs, zero edges, dx, initial_guesses = the
        prediction - None with warm_start=False -, tol, max_iterations, check_every).  Returns soln (N,1,H,W) fp32; with return_info also the
        solver's dict (iterations, converged, relative_residual; a start that already meets tol reports 0 iterations) plus
          prediction_relative_residual  sqrt(sum r^2 / sum f^2) of the prediction per sample, NaN where sum f^2 == 0 (the solver only uses the
                                        prediction's interior, so this is the ||b - A x0|| / ||b|| it starts from when the prediction's edges are 0)
          prediction_max_residual       max|r| per sample
          cold_iterations               with compare_cold=True: the iterations of a second solve started at 0
        A model with boundary_types solves with those edge types and du/dn = 0 on the Neumann edges:
        variable_density_poisson_solve(boundary_types=..., zero data); prediction_relative_residual is then sqrt(sum w r^2 / sum w f^2) over the
        unknowns, r from ops.varcoef_pi_loss_partials with the mask - the ||b - A x0||_W / ||b||_W the solver starts from (all four edges Neumann:
        before its projection of b) - and prediction_max_residual is None unless the model was built with residual_metrics=True: then it is the
        max|r| column of ops.varcoef_error_stats(neumann_mask=...), the same r.
        preconditioner: variable_density_poisson_solve's - 'dst', or 'scaled' for smooth densities; both solves of
        compare_cold use it.
        How many iterations a prediction saves is measured (tools/bench_varcoef_warmstart.py), not promised.  Nothing in the model changes: no
        BatchNormalization update, no gradient, no optimizer state."""
        if not self.density_input:
            raise ValueError('%s.solve() starts the iterative variable-density solve from a prediction and needs density_input=True; the '
                             'constant-coefficient problem is solved directly by dataset.multigrid_poisson_solve, which needs no start' % self.model_name)
        from . import dataset as D
        stack, dx = inputs
        stack, dx = _as_device(stack, self.device), _as_device(dx, self.device)
        pred = self.call([stack, dx], training=False)              # refuses a malformed stack and spacing columns that differ
        d = self._spacing_column(dx).reshape(-1)
        N, _, H, W = stack.shape
        rhs, rho = stack[:, 0].contiguous(), stack[:, 1].contiguous()
        mask = self.neumann_mask
        if mask:
            rr = ops.varcoef_pi_loss_partials(pred.to(torch.float32).contiguous(), rho, rhs, d, mask)
            wi, wj = torch.ones(H, device=self.device), torch.ones(W, device=self.device)        # w on all nodes, 0 on the Dirichlet ones
            wi[0], wi[-1], wj[0], wj[-1] = 0.5 * (mask & 1), 0.5 * (mask >> 1 & 1), 0.5 * (mask >> 2 & 1), 0.5 * (mask >> 3 & 1)
            ff = (torch.outer(wi, wj).double() * rhs.double() ** 2).sum(dim=(1, 2))
            rmax = ops.varcoef_error_stats(pred.to(torch.float32), rho, None, rhs, d, neumann_mask=mask)[:, 6] if self.residual_metrics else None
        else:
            stats = ops.varcoef_error_stats(pred.to(torch.float32), rho, None, rhs, d)
        zero = {k: torch.zeros((N, W if k in ('left', 'right') else H), dtype=torch.float32, device=self.device) for k in ('left', 'right', 'bottom', 'top')}
        kw = dict(tol=tol, max_iterations=max_iterations, check_every=check_every, return_info=True, device=self.device, check_start=True)
        if mask:
            kw['boundary_types'] = self.boundary_types
        if preconditioner != 'dst':
            kw['preconditioner'] = preconditioner
        soln, info = D.variable_density_poisson_solve(rho, rhs, zero, d, initial_guesses=pred if warm_start else None, **kw)
        if not return_info:
            return soln
        if mask:
            s = np.zeros((N, 8))
            s[:, 5], s[:, 7] = rr.cpu().numpy().astype(np.float64), ff.cpu().numpy()
            if rmax is not None:
                s[:, 6] = rmax.cpu().numpy().astype(np.float64)
        else:
            s = stats.cpu().numpy().astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            info['prediction_relative_residual'] = np.where(s[:, 7] > 0, np.sqrt(s[:, 5] / np.where(s[:, 7] > 0, s[:, 7], 1.0)), np.nan)
        info['prediction_max_residual'] = s[:, 6] if (not mask or self.residual_metrics) else None
        if compare_cold:
            info['cold_iterations'] = info['iterations'] if not warm_start else D.variable_density_poisson_solve(rho, rhs, zero, d, **kw)[1]['iterations']
        return soln, info

    def _dummy_batch(self, shape):
        N, H, W = shape
        g = torch.Generator(device='cpu').manual_seed(0)
        rhs = (torch.rand((N, 1, H, W), generator=g) * 2 - 1).to(self.device)
        if self.density_input:                                    # [rhs, rho] with rho in [1, 2]
            rhs = torch.cat([rhs, (torch.rand((N, 1, H, W), generator=g) + 1).to(self.device)], 1)
        return (rhs, torch.full((N, 1), 0.02, device=self.device)), (torch.rand((N, 1, H, W), generator=g) * 0.1).to(self.device)

    def _forward_backward(self, data):
        """forward, loss and backward of one batch (with the reference's gradient accumulation, :275-289): store.flat_g holds the gradient."""
        (rhs, dx), y_true = data
        rhs, dx, y_true = _as_device(rhs, self.device), _as_device(dx, self.device), _as_device(y_true, self.device)
        dx = self._spacing_column(dx)
        S = self.store
        if self.gradient_accumulation_steps is None:
            loss, pred = self._loss_and_grads(rhs, dx, y_true)
            gt = y_true
        else:
            steps = int(self.gradient_accumulation_steps)
            idx = split_indices(rhs.shape[0], steps)
            if self._acc is None:
                self._acc = torch.zeros_like(S.flat_g)
            for s in range(steps):
                a, b = int(idx[s]), int(idx[s + 1])
                loss, pred = self._loss_and_grads(rhs[a:b].contiguous(), dx[a:b].contiguous(), y_true[a:b].contiguous())
                ops.axpby_flat(1.0 / steps, S.flat_g, 0.0 if s == 0 else 1.0, self._acc)     # grads = sum / steps (:287)
                gt = y_true[a:b]
            ops.axpby_flat(1.0, self._acc, 0.0, S.flat_g)
        return loss, gt, pred


# =====================================================================================================================
class _BoundaryTables:
    """The two input-independent device tables of the boundary models (they set spp_levels, x_dir_nmodes, device and the caches _bins, _sinh)."""

    def _bin_table(self, Lh):
        """The spatial pyramid's bins over a boundary of Lh points, as [y0, y1, x0, x1] rows."""
        if Lh not in self._bins:
            bins = []
            for lv in self.spp_levels:
                ix = split_indices(Lh, lv)
                if (np.diff(ix) <= 0).any():
                    raise ValueError('boundary too short for the spatial pyramid: %d bins over %d points' % (lv, Lh))
                bins += [[0, 1, ix[b], ix[b + 1]] for b in range(lv)]
            self._bins[Lh] = torch.tensor(np.array(bins, dtype=np.int32), device=self.device)
        return self._bins[Lh]

    def _sinh_table(self, X):
        """build_series_x_dir_components (Dirichlet_BC_NN_Legacy.py:106-111, Dirichlet_BC_NN_Metalearning.py:103-110): input-independent, so
        tabulated on the host (fp64, rounded once)."""
        if X not in self._sinh:
            xbar = np.linspace(0.0, 1.0, X)
            v = np.sinh(np.outer(np.arange(1, self.x_dir_nmodes + 1, dtype=np.float64), np.pi * (xbar - 1.0)))
            v = v / np.abs(v).max(axis=1, keepdims=True)
            self._sinh[X] = torch.from_numpy(v.astype(np.float32)).to(self.device).contiguous()
        return self._sinh[X]


class Dirichlet_BC_NN_Legacy_2(_BoundaryTables, _ModelBase):
    """Drop-in for poisson_CNN/models/Dirichlet_BC_NN_Legacy.py:14-187: same constructor kwargs (the "model" section of
    experiments/dbcnn.json loads unchanged), `model([bc (N,1,L), dx (N,1), x_output_resolution]) -> (N,1,X,L)`,
    `train_step(((bc, dx), y))`.  1-D tensors are NHWC (N,1,L,C) inside; Conv1D kernels are stored as (1,k,Cin,Cout)."""
    model_name = 'Dirichlet_BC_NN_Legacy_2'

    def __init__(self, data_format='channels_first', boundary_conv_config=None, spp_config=None, domain_info_mlp_config=None,
                 final_convolutions_config=None, postsmoother_iterations=0, use_batchnorm=False, device=None, seed=0, batchnorm_training=False):
        if data_format not in ('channels_first', 'channels_last'):
            raise ValueError('data_format must be channels_first or channels_last')
        if boundary_conv_config is None:
            raise ValueError('Provide a config for the boundary convolutions.')
        if spp_config is None:
            raise ValueError('Provide a config for the Spatial Pyramid Pooling.')
        if final_convolutions_config is None:
            raise ValueError('Provide a config for the domain convolutions.')
        if domain_info_mlp_config is None:
            raise ValueError('Provide a config for the domain info MLP.')
        self._init_device(device, _CPU_NOTE_RAISES)
        self.ndims, self.data_format, self.use_batchnorm = 2, data_format, use_batchnorm
        assert boundary_conv_config['filters'][-1] == domain_info_mlp_config['units'][-1]       # reference :39
        self.x_dir_nmodes = M = domain_info_mlp_config['units'][-1]
        if M > 27:
            import warnings
            warnings.warn('%d sinh modes chosen may lead to NaN values with float32 precision. Consider using fewer than 28 when using float32.' % M)
        self.store = S = L.ParamStore()
        S.bn_training = bool(batchnorm_training)
        self.ctx = C = L.Context()
        C.enable_side_stream()
        # boundary convolutions (:44-63): per stage conv (+BN) then a 1-D resnet
        bcc = copy.deepcopy(boundary_conv_config)
        mode, val = bcc.pop('padding_mode', 'CONSTANT'), bcc.pop('constant_padding_value', 0.0)
        self.boundary = []
        cin = 3
        for k in range(len(bcc['filters'])):
            a = get_init_arguments_from_config(bcc, k, ['filters', 'kernel_sizes'], ['filters', 'kernel_size'])
            act, ub = a.get('activation', 'linear'), a.get('use_bias', True)
            self.boundary.append(L.ConvUnit(S, C, 'bc/stage%d/conv' % k, (1, a['kernel_size']), cin, a['filters'], padding_mode=mode, pad_value=val,
                                            activation=act, use_bias=ub, bn_name=('bc/stage%d/bn' % k) if use_batchnorm else None))
            self.boundary.append(L.resnet(S, C, 'bc/stage%d/res' % k, a['filters'], (1, a['kernel_size']), use_batchnorm=use_batchnorm,
                                          padding_mode=mode, constant_padding_value=val, activation=act, use_bias=ub))
            cin = a['filters']
        # SPP (:68) + domain-info MLP (:69-74)
        self.spp_levels = [lv if isinstance(lv, int) else lv[0] for lv in spp_config['levels']]
        kind = spp_config.get('pooling_type', 'average').lower()
        if kind not in ('average', 'avg', 'max'):
            raise ValueError('spp_config pooling_type must be "average" or "max" (layers/SpatialPyramidPool.py:17-24)')
        self.spp_max = kind == 'max'
        din = 3 + sum(self.spp_levels)
        self.mlp = []
        for k, (u, a) in enumerate(zip(domain_info_mlp_config['units'], domain_info_mlp_config['activations'])):
            self.mlp.append(L.Dense(S, 'mlp/dense%d' % k, din, u, a))
            din = u
        # final convolutions (:76-97)
        fc = copy.deepcopy(final_convolutions_config)
        nst = len(fc['filters'])
        fmode, fval = fc.pop('padding_mode', 'CONSTANT'), fc.pop('constant_padding_value', 0.0)
        nreg = fc.pop('final_regular_conv_stages', 2)
        self.final = []
        cin = M + 2
        for k in range(nst - nreg):
            a = get_init_arguments_from_config(fc, k, ['filters', 'kernel_sizes'], ['filters', 'kernel_size'])
            act, ub = a.get('activation', 'linear'), a.get('use_bias', True)
            self.final.append(L.ConvUnit(S, C, 'final/stage%d/conv' % k, a['kernel_size'], cin, a['filters'], padding_mode=fmode, pad_value=fval,
                                         activation=act, use_bias=ub))
            self.final.append(L.resnet(S, C, 'final/stage%d/res' % k, a['filters'], a['kernel_size'], padding_mode='constant', activation=act, use_bias=ub))
            cin = a['filters']
        for j, k in enumerate(range(nst - nreg, nst)):
            self.final.append(L.ConvUnit(S, C, 'final/out%d' % j, fc['kernel_sizes'][k], cin, fc['filters'][k], pad='same', activation='tanh',
                                         use_bias=fc.get('use_bias', True)))
            cin = fc['filters'][k]
        if cin != 1:
            raise ValueError('the last final convolution must have 1 filter')
        self.postsmoother = L.JacobiIterationLayer(postsmoother_iterations) if postsmoother_iterations > 0 else None
        S.finalize(self.device)
        S.initialize(seed)
        self._bins, self._sinh = {}, {}

    def call(self, inp, training=False):
        """reference :126-170."""
        bc, dx, X = inp
        X = int(X)
        bc, dx = _as_device(bc, self.device), _as_device(dx, self.device)
        if bc.dim() != 3 or bc.shape[1] != 1:
            raise ValueError('bc must have shape (N,1,L)')
        dx = _dx_column(dx)
        N, _, Lh = bc.shape
        S = self.store
        S.refresh_bn()
        bc2 = bc.reshape(N, Lh)
        o = ops.dbc_assemble_input(bc2)
        hint = None
        for lyr in self.boundary:
            o = lyr.forward(o, training=training, x_absmax=hint)
            hint = lyr.out_absmax
        bc_conv = o                                                            # (N,1,L,M)
        bins = self._bin_table(Lh)
        spp_arg = None
        if self.spp_max:
            feats, spp_arg = ops.spp_max_fwd(bc_conv.contiguous(), bins)
        else:
            feats = ops.spp_avg_fwd(bc_conv, bins)
        ds = torch.cat([dx * float(X - 1), dx * float(Lh - 1)], 1)           # compute_domain_sizes (:131); tiny (N,2) host-side assembly
        d = torch.cat([dx, ds / ds.amax(dim=1, keepdim=True), feats], 1).contiguous()
        for lyr in self.mlp:
            d = lyr.forward(d, training=training)
        sh = self._sinh_table(X)
        x = ops.dbc_expand_fwd(bc_conv, sh, d)                                # (N,X,L,M+2)
        hint = None
        for lyr in self.final:
            x = lyr.forward(x, training=training, x_absmax=hint)
            hint = lyr.out_absmax
        pre = x.view(N, X, Lh)
        out, _ = ops.set_max_magnitude_fwd(pre, 1.0)                          # (:163)
        ops.set_first_row(out, bc2)                                           # (:165-166)
        if training:
            self._saved = {'bc_conv': bc_conv, 'mlp_out': d, 'sinh': sh, 'pre': pre, 'bins': bins, 'spp_arg': spp_arg, 'shape': (N, X, Lh)}
        if self.postsmoother is not None:
            out = self.postsmoother.forward(out.view(N, X, Lh, 1), torch.zeros_like(out).view(N, X, Lh, 1), _dx_pair(dx), training=training).view(N, X, Lh)
        return out.view(N, 1, X, Lh)

    def backward(self, dpred):
        sv = self._saved
        self._saved = None
        N, X, Lh = sv['shape']
        d = dpred.contiguous().view(N, X, Lh)
        if self.postsmoother is not None:
            d = self.postsmoother.backward(d.view(N, X, Lh, 1)).view(N, X, Lh)
        else:
            d = d.clone()
        ops.set_first_row(d, None)                                            # the first row is the (constant) boundary input
        d = ops.set_max_magnitude_bwd(sv['pre'], d, 1.0).view(N, X, Lh, 1)
        for lyr in reversed(self.final):
            d = lyr.backward(d, inplace=True)
        dbc_conv, dd = ops.dbc_expand_bwd(d, sv['bc_conv'], sv['sinh'], sv['mlp_out'], ws=self.ctx.ws)
        for lyr in reversed(self.mlp):
            dd = lyr.backward(dd, need_dx=True)
        dfeats = dd[:, 3:].contiguous()                                       # [dx, domain sizes] carry no parameters upstream
        dspp = (ops.spp_max_bwd(sv['spp_arg'], dfeats, tuple(sv['bc_conv'].shape)) if self.spp_max
                else ops.spp_avg_bwd(sv['bins'], dfeats, tuple(sv['bc_conv'].shape)))
        dbc_conv = ops.axpby(1.0, dspp, 1.0, dbc_conv)
        d = dbc_conv
        for i, lyr in enumerate(reversed(self.boundary)):
            last = i == len(self.boundary) - 1
            d = lyr.backward(d, need_dx=not last, inplace=True) if isinstance(lyr, L.ConvUnit) else lyr.backward(d, inplace=True)
        self.ctx.join()                                            # weight gradients of the side stream
        self.store.finish_bn_grads()

    def _forward_backward(self, data):
        """reference :172-187: the loss sees rhs = 0 and dx repeated for both axes."""
        (bc, dx), y_true = data
        bc, dx, y_true = _as_device(bc, self.device), _as_device(dx, self.device), _as_device(y_true, self.device)
        dx = _dx_column(dx)
        pred = self.call([bc, dx, y_true.shape[2]], training=True)
        loss, dpred = self.loss_fn.value_and_grad(y_true, pred, torch.zeros_like(y_true), _dx_pair(dx))
        self.backward(dpred)
        return loss, y_true, pred

    # ------------------------------------------------------------------ used by Poisson_CNN_Legacy: several calls per step share the weights
    def _stateful(self):
        objs = [self]
        for lyr in self.boundary + self.final:
            objs += [lyr.c0, lyr.c1, lyr.c2] if isinstance(lyr, L.resnet) else [lyr]
        return objs + self.mlp + ([self.postsmoother] if self.postsmoother is not None else [])

    def snapshot(self):
        """What backward() needs from the last call(training=True)."""
        return [(o, {k: getattr(o, k) for k in ('saved', '_saved', 'dx2') if hasattr(o, k)}) for o in self._stateful()]

    @staticmethod
    def restore(snap):
        for o, attrs in snap:
            for k, v in attrs.items():
                setattr(o, k, v)


# =====================================================================================================================
class Poisson_CNN_Legacy(_ModelBase):
    """Drop-in for poisson_CNN/models/Poisson_CNN_Legacy.py:5-71: `Poisson_CNN_Legacy(hpnn, dbcnn)`,
    `model([rhs (N,1,H,W), left (N,1,W), top (N,1,H), right (N,1,W), bottom (N,1,H), dx (N,1)]) -> (N,1,H,W)`: the homogeneous
    solution plus one Dirichlet_BC_NN_Legacy_2 pass per edge (left/right and top/bottom are batched: same weights, same shapes),
    rotated/flipped into place by flip_and_rotate_tensor and un-normalised by the per-sample scaling factors."""
    model_name = 'Poisson_CNN_Legacy'

    def __init__(self, hpnn, dbcnn, jacobi_iterations=0):
        if jacobi_iterations > 0:
            # the reference constructor dereferences an unimported module name here (Poisson_CNN_Legacy.py:11) and raises NameError
            raise NotImplementedError('Poisson_CNN_Legacy: jacobi_iterations > 0 is unreachable in the reference (NameError at construction)')
        if getattr(hpnn, 'density_input', False):
            raise NotImplementedError('Poisson_CNN_Legacy around a density_input model is not built: the boundary network solves the constant-coefficient '
                                      'problem - construct the Homogeneous_Poisson_NN_Legacy with density_input=False')
        self.hpnn, self.dbcnn = hpnn, dbcnn
        self._init_device(hpnn.device)
        self.data_format = getattr(hpnn, 'data_format', 'channels_first')

    # weights: the two sub-models' lists, hpnn first (Keras tracks attributes in assignment order)
    @property
    def stores(self):
        return [self.hpnn.store, self.dbcnn.store]

    @property
    def weight_names(self):
        return ['hpnn/' + n for n in self.hpnn.weight_names] + ['dbcnn/' + n for n in self.dbcnn.weight_names]

    @property
    def trainable_variables(self):
        return self.hpnn.trainable_variables + self.dbcnn.trainable_variables

    def get_weights(self):
        return self.hpnn.get_weights() + self.dbcnn.get_weights()

    def set_weights(self, weights):
        if isinstance(weights, dict):
            self.hpnn.set_weights({n[5:]: v for n, v in weights.items() if n.startswith('hpnn/')})
            self.dbcnn.set_weights({n[6:]: v for n, v in weights.items() if n.startswith('dbcnn/')})
        else:
            k = len(self.hpnn.weight_names)
            self.hpnn.set_weights(list(weights[:k]))
            self.dbcnn.set_weights(list(weights[k:]))

    def count_params(self):
        return self.hpnn.count_params() + self.dbcnn.count_params()

    def summary(self, print_fn=print):
        self.hpnn.summary(print_fn)
        self.dbcnn.summary(print_fn)

    # (transpose, flip rows, flip columns) that flip_and_rotate_tensor applies to each edge's result (:36-46) ...
    _PLACE = {'left': (False, False, False), 'top': (True, False, True), 'right': (False, True, False), 'bottom': (True, False, False)}
    # ... and their adjoints (a transpose swaps the roles of the two flips)
    _ADJ = {'left': (False, False, False), 'top': (True, True, False), 'right': (False, True, False), 'bottom': (True, False, False)}

    def call(self, inp, training=False):
        rhs, left, top, right, bottom, dx = [_as_device(v, self.device) for v in inp]
        dx = _dx_column(dx)
        N, _, H, W = rhs.shape
        rhs_n, rhs_f = ops.set_max_magnitude_fwd(rhs.reshape(N, H * W), 1.0)                 # :24
        edges = {}
        for name, v in (('left', left), ('top', top), ('right', right), ('bottom', bottom)):
            edges[name] = ops.set_max_magnitude_fwd(v.reshape(N, -1), 1.0)                   # :25-28
        h = self.hpnn.call([rhs_n.view(N, 1, H, W), dx], training=training)
        dmax = torch.cat([dx * float(H - 1), dx * float(W - 1)], 1).amax(dim=1)
        scale_h = (dmax * dmax / rhs_f).contiguous()                                          # :30
        pred = ops.flip_rotate(h.view(N, H, W), alpha=scale_h)
        dx2 = torch.cat([dx, dx], 0).contiguous()
        snaps, scales = {}, {}
        for pair, X in ((('left', 'right'), H), (('top', 'bottom'), W)):
            bc = torch.cat([edges[pair[0]][0], edges[pair[1]][0]], 0)
            out = self.dbcnn.call([bc.view(2 * N, 1, -1), dx2, X], training=training)        # (2N,1,X,L)
            out = out.view(2 * N, X, -1)
            for j, name in enumerate(pair):
                scales[name] = (1.0 / edges[name][1]).contiguous()                            # :33-46
                t, fy, fx = self._PLACE[name]
                ops.flip_rotate(out[j * N:(j + 1) * N], transpose=t, flip_y=fy, flip_x=fx, alpha=scales[name], out=pred, accumulate=True)
            if training:
                snaps[pair] = self.dbcnn.snapshot()
        if training:
            self._saved = {'snaps': snaps, 'scales': scales, 'scale_h': scale_h, 'shape': (N, H, W)}
        return pred.view(N, 1, H, W)

    def backward(self, dpred):
        sv = self._saved
        self._saved = None
        N, H, W = sv['shape']
        d = dpred.contiguous().view(N, H, W)
        self.hpnn.backward(ops.flip_rotate(d, alpha=sv['scale_h']).view(N, 1, H, W))
        acc = None
        for pair, X in ((('top', 'bottom'), W), (('left', 'right'), H)):
            Lh = H if X == W else W
            dout = ops.empty((2 * N, X, Lh), self.device)
            for j, name in enumerate(pair):
                t, fy, fx = self._ADJ[name]
                ops.flip_rotate(d, transpose=t, flip_y=fy, flip_x=fx, alpha=sv['scales'][name], out=dout[j * N:(j + 1) * N])
            self.dbcnn.restore(sv['snaps'][pair])
            self.dbcnn.backward(dout.view(2 * N, 1, X, Lh))
            g = self.dbcnn.store.flat_g
            if acc is None:
                acc = g.clone()
            else:
                ops.axpby_flat(1.0, acc, 1.0, g)                                              # the two passes share the weights

    def _forward_backward(self, data):
        """reference :56-66."""
        inputs, y_true = data
        inputs = [_as_device(v, self.device) for v in inputs]
        y_true = _as_device(y_true, self.device)
        pred = self.call(inputs, training=True)
        loss, dpred = self.loss_fn.value_and_grad(y_true, pred, inputs[0], _dx_pair(_dx_column(inputs[5])))
        self.backward(dpred)
        return loss, y_true, pred
