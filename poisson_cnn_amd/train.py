"""Optimizers, callbacks and the training entry point (drop-in for poisson_CNN/train/hpnn_legacy_train.py and train/utils.py).

python -m poisson_cnn_amd.train config.json [--checkpoint_dir D] [--continue_from_checkpoint D] [--dataset_type analytical|analytical_mixed|numerical|variable_density|
                                            variable_density_analytical] [--learning_rate X|from_json]
Under `torchrun` (WORLD_SIZE > 1) the batch is sharded over ranks and gradients are all-reduced over RCCL
(parallel.DataParallel), replacing the reference's tf.distribute.MirroredStrategy (train/hpnn_legacy_train.py:37-38).
`analytical_mixed` (extension): the analytic generator with a boundary type per edge, for a Homogeneous_Poisson_NN_Legacy whose bc_type is a dict.
`variable_density` (extension): dataset.variable_density_dataset_generator, div((1/rho) grad u) = f with the input stack [rhs, rho], for
--model hpnn with "density_input": true in the model section; the config's loss is then built as losses.variable_density_loss_wrapper.
"boundary_types" and "residual_metrics" in that model section reach the model as its keywords of the same names; "preconditioner" ('dst' |
'scaled') and "density_profile" ('abs' | 'smooth') in the dataset section, when present, reach the generator as its keywords of the same names.
`variable_density_analytical` (extension): dataset.reverse_variable_density_dataset_generator, the same problem, model, loss and consistency rules
with solve-free data - a random series u, a random rho and the discrete right-hand side L_h(rho) u from one launch; its
dataset section takes "fourier_coeff_grid_size_range" in place of the solver's keywords.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import ops


_CLIP_OPTIONS = ('clipnorm', 'global_clipnorm', 'clipvalue', 'decay')


class _Optimizer:
    """What Adam and SGD share: the parameter buckets they are bound to and the tf.keras OptimizerV2 options `clipnorm`, `global_clipnorm`,
    `clipvalue`, `decay` (TF 2.4; formulas in include/pcnn.h, kernels in csrc/grad_clip.hip) and `lr` as an alias of `learning_rate`.

    A clip option rewrites every bucket's gradient in place in front of the update (per bucket: squared norms, scales, apply), which then runs
    with grad_scale = 1; with no option set apply_gradients launches exactly the update kernels.  `decay` changes only the learning rate handed
    down: lr / (1 + decay * t), t = updates already applied; `learning_rate` stays the base value ReduceLROnPlateau reads and writes.
    `global_norm`: a device scalar, the pre-clip global gradient norm of the last step while a clip option is set."""

    def _init_options(self, who, learning_rate, kwargs):
        kwargs = dict(kwargs)
        if 'lr' in kwargs:
            learning_rate = kwargs.pop('lr')
        opts = {k: kwargs.pop(k, None) for k in _CLIP_OPTIONS}
        _reject_unsupported_optimizer_kwargs(who, kwargs)
        for k, v in opts.items():
            if v is not None and not float(v) >= 0.0:
                raise ValueError('%s: %s must be >= 0, got %r' % (who, k, v))
        if opts['clipnorm'] is not None and opts['global_clipnorm'] is not None:
            raise ValueError('%s: clipnorm and global_clipnorm cannot both be set' % who)
        self.clipnorm, self.global_clipnorm, self.clipvalue = (None if opts[k] is None else float(opts[k]) for k in _CLIP_OPTIONS[:3])
        self.decay = float(opts['decay'] or 0.0)
        self.learning_rate = float(learning_rate)
        self.iterations = 0
        self.global_norm = None

    @property
    def clip_mode(self):
        return 'clipnorm' if self.clipnorm is not None else 'global_clipnorm' if self.global_clipnorm is not None else None

    @property
    def clips(self):
        return self.clip_mode is not None or self.clipvalue is not None

    def decayed_learning_rate(self, t=None):
        """The learning rate of the update after `t` applied ones (default: the next one)."""
        t = self.iterations if t is None else t
        return self.learning_rate / (1.0 + self.decay * t) if self.decay else self.learning_rate

    def bind(self, store):
        """store: one ParamStore or a list of them (a composite model such as Poisson_CNN_Legacy trains several buckets)."""
        self.stores = list(store) if isinstance(store, (list, tuple)) else [store]
        self.store = self.stores[0]
        if self.clips:
            self._plans = [ops.grad_clip_plan(store_variable_sizes(s)) for s in self.stores]
            dev = self.store.flat_g.device
            self._totals = torch.zeros(len(self.stores), dtype=torch.float64, device=dev)      # one squared norm per bucket, in binding order
            self._global_scale = torch.ones(1, dtype=torch.float32, device=dev)
            self.global_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._init_state()

    def _init_state(self):
        pass

    def _clip_gradients(self, grad_scale):
        """Norms of every bucket, then the scales (global mode: ONE launch over the buckets' totals, no host round trip), then the in-place clip."""
        mode, pairs = self.clip_mode, list(zip(self.stores, self._plans))
        for k, (s, plan) in enumerate(pairs):
            ops.grad_sqnorms(s.flat_g, plan, grad_scale, total=self._totals[k:k + 1])
        if mode == 'clipnorm':
            for k, (s, plan) in enumerate(pairs):
                ops.grad_clip_scales(plan, mode, self.clipnorm, totals=self._totals, global_norm=self.global_norm if k == 0 else None)
        else:
            ops.grad_clip_scales(self._plans[0], mode, self.global_clipnorm or 0.0, totals=self._totals, scale=self._global_scale, global_norm=self.global_norm)
        for s, plan in pairs:
            ops.grad_clip_apply(s.flat_g, plan, mode, scale=plan.scale if mode == 'clipnorm' else self._global_scale, clipvalue=self.clipvalue,
                                grad_scale=grad_scale)

    def apply_gradients(self, grad_scale=1.0):
        lr = self.decayed_learning_rate()
        if self.clips:
            self._clip_gradients(grad_scale)
            grad_scale = 1.0
        self.iterations += 1
        self._update(lr, grad_scale)


def store_variable_sizes(store):
    """Element counts of a ParamStore's trainable variables in the physical order of flat_g: the 'w' specs, then every BN gamma, then every BN beta
    (layers.ParamStore.finalize).  Moving statistics are not variables."""
    by_kind = {k: [int(np.prod(shape)) for _, shape, _, kind in store.specs if kind == k] for k in ('w', 'bn_gamma', 'bn_beta')}
    return by_kind['w'] + by_kind['bn_gamma'] + by_kind['bn_beta']


def _reject_unsupported_optimizer_kwargs(who, kwargs):
    """Whatever is left after the options _Optimizer implements: an option that would change the update must not be swallowed silently - a
    config that sets it would train differently from the reference."""
    for k, v in kwargs.items():
        raise NotImplementedError('%s: optimizer option %r=%r is not implemented' % (who, k, v))


class Adam(_Optimizer):
    """tf.keras.optimizers.Adam defaults (train/utils.py:3-8; experiments/hpnn.json optimizer_parameters)."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name='Adam', **kwargs):
        self._init_options('Adam', learning_rate, kwargs)
        self.amsgrad = bool(amsgrad)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def _init_state(self):
        self.ms = [torch.zeros_like(s.flat_w) for s in self.stores]
        self.vs = [torch.zeros_like(s.flat_w) for s in self.stores]
        self.vhats = [torch.zeros_like(s.flat_w) if self.amsgrad else None for s in self.stores]
        self.m, self.v = self.ms[0], self.vs[0]

    def _update(self, lr, grad_scale):
        for s, m, v, vh in zip(self.stores, self.ms, self.vs, self.vhats):
            ops.adam_step(s.flat_w, s.flat_g, m, v, lr, self.beta_1, self.beta_2, self.epsilon, self.iterations, grad_scale, vhat=vh)


class SGD(_Optimizer):
    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name='SGD', **kwargs):
        self._init_options('SGD', learning_rate, kwargs)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)

    def _init_state(self):
        self.vs = [torch.zeros_like(s.flat_w) for s in self.stores] if self.momentum != 0.0 else None

    def _update(self, lr, grad_scale):
        for k, s in enumerate(self.stores):
            if self.momentum != 0.0:
                ops.sgd_momentum_step(s.flat_w, s.flat_g, self.vs[k], lr, self.momentum, self.nesterov, grad_scale)
            else:
                ops.sgd_step(s.flat_w, s.flat_g, lr, grad_scale)


def choose_optimizer(name):
    """train/utils.py:3-8."""
    name = name.lower()
    if name == 'adam':
        return Adam
    if name == 'sgd':
        return SGD
    raise ValueError('unknown optimizer ' + name)


# ----------------------------------------------------------------------------- Keras-like callbacks (train/hpnn_legacy_train.py:46-50)
class Callback:
    def set_model(self, model):
        self.model = model

    def on_batch_end(self, batch, logs):
        pass

    def on_epoch_end(self, epoch, logs):
        pass


class ModelCheckpoint(Callback):
    def __init__(self, filepath, save_weights_only=True, save_best_only=True, monitor='loss', save_format=None):
        self.filepath, self.best, self.monitor, self.save_best_only = filepath, math.inf, monitor, save_best_only
        self.save_format = save_format                       # None: flat .npz; 'tf': TensorFlow checkpoint files (tf_checkpoint.py)

    def on_epoch_end(self, epoch, logs):
        v = logs[self.monitor]
        if not self.save_best_only or v < self.best:
            self.best = min(self.best, v)
            if int(os.environ.get('RANK', '0')) == 0:
                self.model.save_weights(self.filepath, **({'save_format': self.save_format} if self.save_format else {}))


class ReduceLROnPlateau(Callback):
    """tf.keras.callbacks.ReduceLROnPlateau, mode 'min' (train/hpnn_legacy_train.py:48 passes patience and min_lr; everything else is
    the Keras default: factor 0.1, min_delta 1e-4, cooldown 0).  An epoch counts as an improvement only if monitor < best - min_delta.
    The monitored value is what fit() hands to on_epoch_end: the last batch's (global) loss, as in Keras."""

    def __init__(self, monitor='loss', factor=0.1, patience=10, verbose=0, mode='auto', min_delta=1e-4, cooldown=0, min_lr=0.0):
        if factor >= 1.0:
            raise ValueError('ReduceLROnPlateau does not support a factor >= 1.0.')
        if mode not in ('auto', 'min'):
            raise NotImplementedError("ReduceLROnPlateau: only mode 'min' / 'auto' on a loss is implemented")
        self.monitor, self.factor, self.patience, self.verbose = monitor, factor, patience, verbose
        self.min_delta, self.cooldown, self.min_lr = min_delta, cooldown, min_lr
        self.best, self.wait, self.cooldown_counter = math.inf, 0, 0

    def on_epoch_end(self, epoch, logs):
        current = logs[self.monitor]
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if current < self.best - self.min_delta:
            self.best, self.wait = current, 0
        elif self.cooldown_counter <= 0:
            self.wait += 1
            if self.wait >= self.patience:
                opt = self.model.optimizer
                if opt.learning_rate > self.min_lr:
                    opt.learning_rate = max(opt.learning_rate * self.factor, self.min_lr)
                    if self.verbose:
                        print('Epoch %d: ReduceLROnPlateau reducing learning rate to %g.' % (epoch + 1, opt.learning_rate))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class EarlyStopping(Callback):
    """tf.keras.callbacks.EarlyStopping (same arguments, Keras' order).  An epoch improves when monitor < best - min_delta (mode 'min'; 'auto'
    is 'max' for a monitor with 'acc' in its name, else 'min') or monitor > best + min_delta ('max'); `best` starts at `baseline` when given.
    Once `wait`, the number of epochs without improvement since the last one, reaches `patience` (checked from the first non-improving
    epoch on, so patience=0 stops like patience=1), model.stop_training is set.  An epoch whose logs lack the
    monitored key (validation_freq > 1) is skipped.
    restore_best_weights keeps a device copy of every store's flat_w (and flat_stats) of the best epoch and, when it stops the training,
    writes them back and calls ops.weights_changed().  A new fit() (set_model) starts the bookkeeping afresh."""

    def __init__(self, monitor='val_loss', min_delta=0, patience=0, verbose=0, mode='auto', baseline=None, restore_best_weights=False):
        if mode not in ('auto', 'min', 'max'):
            raise ValueError("EarlyStopping mode must be 'auto', 'min' or 'max', got %r" % (mode,))
        if mode == 'auto':
            mode = 'max' if 'acc' in monitor else 'min'
        self.monitor, self.patience, self.verbose, self.mode, self.baseline = monitor, int(patience), verbose, mode, baseline
        self.min_delta = abs(float(min_delta))
        self.restore_best_weights = bool(restore_best_weights)
        self._reset()

    def _reset(self):
        self.wait, self.stopped_epoch, self.best_weights = 0, 0, None
        self.best = self.baseline if self.baseline is not None else (math.inf if self.mode == 'min' else -math.inf)

    def set_model(self, model):
        self.model = model
        self._reset()

    def _improved(self, current):
        return current + self.min_delta < self.best if self.mode == 'min' else current - self.min_delta > self.best

    def _stores(self):
        return list(self.model.stores) if hasattr(self.model, 'stores') else [self.model.store]

    def on_epoch_end(self, epoch, logs):
        current = logs.get(self.monitor)
        if current is None:
            return
        if self._improved(current):
            self.best, self.wait = current, 0
            if self.restore_best_weights:
                self.best_weights = [(s.flat_w.clone(), s.flat_stats.clone() if getattr(s, 'flat_stats', None) is not None else None) for s in self._stores()]
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.verbose:
                print('Epoch %d: early stopping' % (epoch + 1))
            if self.restore_best_weights and self.best_weights is not None:
                for s, (w, stats) in zip(self._stores(), self.best_weights):
                    s.flat_w.copy_(w)
                    if stats is not None:
                        s.flat_stats.copy_(stats)
                ops.weights_changed()


class TerminateOnNaN(Callback):
    def on_batch_end(self, batch, logs):
        if not math.isfinite(logs['loss']):
            print('Batch %d: Invalid loss, terminating training' % batch)
            self.model.stop_training = True


def latest_checkpoint(checkpoint_dir):
    """tf.train.latest_checkpoint: the prefix named by `model_checkpoint_path` in <dir>/checkpoint, or None."""
    state = os.path.join(checkpoint_dir, 'checkpoint')
    if os.path.exists(state):
        for line in open(state):
            if line.startswith('model_checkpoint_path:'):
                name = line.split(':', 1)[1].strip().strip('"')
                return name if os.path.isabs(name) else os.path.join(checkpoint_dir, name)
    return None


def load_model_checkpoint(model, checkpoint_path, **unused):
    """train/utils.py:10-29.  A directory holding TensorFlow checkpoint files (a `checkpoint` state file naming the prefix, as Keras'
    ModelCheckpoint leaves it) is read through tf_checkpoint.py; otherwise the flat .npz this package writes by default."""
    if checkpoint_path is not None:
        path = checkpoint_path
        if os.path.isdir(path):
            path = latest_checkpoint(path) or os.path.join(path, 'chkpt.checkpoint.npz')
        print('Attempting to load checkpoint from ' + path)
        model.load_weights(path)


_DENSITY_DATASET_TYPES = ('variable_density', 'variable_density_analytical')      # the dataset types behind a "density_input" model


def main(argv=None):
    from . import configs
    from .utils import convert_tf_object_names, neumann_flags
    from .models import Homogeneous_Poisson_NN_Legacy, Dirichlet_BC_NN_Legacy_2, Poisson_CNN_Legacy
    from .losses import loss_wrapper, variable_density_loss_wrapper
    from .dataset import (numerical_dataset_generator, reverse_poisson_dataset_generator, reverse_poisson_dataset_generator_homogeneous_neumann,
                          reverse_poisson_dataset_generator_mixed, reverse_variable_density_dataset_generator, variable_density_dataset_generator)
    from . import parallel
    p = argparse.ArgumentParser(description='Train the Homogeneous Poisson NN')
    p.add_argument('config', type=str)
    p.add_argument('--checkpoint_dir', type=str, default='.')
    p.add_argument('--continue_from_checkpoint', type=str, default=None)
    p.add_argument('--dataset_type', type=lambda x: str(x).lower(), default='analytical')
    p.add_argument('--learning_rate', type=str, default=None)
    p.add_argument('--epochs', type=int, default=None)
    p.add_argument('--model', type=lambda x: str(x).lower(), default='hpnn', choices=['hpnn', 'dbcnn', 'pcnn', 'unet', 'dbcnn_rnn'],
                   help='hpnn: train/hpnn_legacy_train.py (train/hpnn_train.py when the model section carries model_type); dbcnn: train/dbcnn_legacy_train.py; '
                        'pcnn: train/pcnn_end_to_end.py; unet: train/UNet.py; dbcnn_rnn: train/dbcnn_rnn_train.py')
    args = p.parse_args(argv)
    if args.dataset_type not in ('numerical', 'analytical', 'analytical_mixed') + _DENSITY_DATASET_TYPES:
        raise ValueError('Invalid dataset type. Received: ' + args.dataset_type)
    config = convert_tf_object_names(configs.load_config(args.config))
    msec = config.get('model', {})
    density_model = bool(msec.get('density_input', False))
    density_data = args.dataset_type in _DENSITY_DATASET_TYPES      # both yield the stack [rhs, rho] and share every consistency rule below
    flag = '--dataset_type ' + args.dataset_type
    if density_data and (args.model != 'hpnn' or 'model_type' in msec or not density_model):
        raise ValueError('%s yields the two-channel input [rhs, rho]: it needs --model hpnn and "density_input": true in the '
                         "config's model section (got --model %s, density_input %r)" % (flag, args.model, msec.get('density_input', False)))
    if density_data and config.get('dataset', {}).get('boundaries', 'zero') != 'zero':
        raise ValueError("%s trains the homogeneous model: it needs boundaries 'zero' in the dataset section (got %r; with "
                         "'random' the generator yields the four edge arrays as further inputs, which no model here reads) - drop the key or set it to "
                         "'zero'" % (flag, config['dataset']['boundaries'],))
    model_bt = msec.get('boundary_types') if density_model else None
    if density_data and model_bt is not None:
        # the model, its loss and the generator's ground truth share one set of edge types: the dataset section names the same ones or none
        if not isinstance(model_bt, dict):
            raise ValueError("the model section's boundary_types is a dict edge -> 'dirichlet' | 'neumann', got %r" % (model_bt,))
        dsec = config.setdefault('dataset', {})
        if dsec.get('boundary_types') is None:
            dsec['boundary_types'] = dict(model_bt)
        elif neumann_flags(dsec['boundary_types']) != neumann_flags(model_bt):
            raise ValueError('%s: the model section has boundary_types %r and the dataset section %r - the ground truth '
                             'must be solved with the edge types the model and its loss use; make the two equal or drop the dataset section\'s'
                             % (flag, model_bt, dsec['boundary_types']))
    elif density_data and any(neumann_flags(config.get('dataset', {}).get('boundary_types'))):
        raise ValueError('%s with Neumann boundary_types %r in the dataset section: the solver and the generator take '
                         'per-edge Neumann boundaries, but the model does not - Homogeneous_Poisson_NN_Legacy(density_input=True) has no Neumann bc_type and '
                         'its flux-form loss and smoother keep every edge fixed; drop boundary_types, or give the model section the same '
                         '"boundary_types" (the keyword of the variable-density model, loss and smoother)' % (flag, config['dataset']['boundary_types'],))
    if density_model and not density_data:
        raise ValueError('a model with "density_input": true reads the stack [rhs, rho], which only --dataset_type variable_density and '
                         'variable_density_analytical yield (got --dataset_type %s): pass one of the two or drop density_input from the model section'
                         % args.dataset_type)
    if args.dataset_type == 'analytical_mixed' and (args.model != 'hpnn' or 'model_type' in config['model']
                                                    or not isinstance(config['model'].get('bc_type'), dict)):
        raise ValueError('--dataset_type analytical_mixed is the per-edge analytic generator of Homogeneous_Poisson_NN_Legacy: it needs --model hpnn and '
                         'a model bc_type that is a dict over left/right/bottom/top (got --model %s, bc_type %r)' % (args.model, config['model'].get('bc_type')))
    if config['training'].get('precision', 'float32') != 'float32':
        raise NotImplementedError('the HIP kernels compute in float32')
    dp = parallel.DataParallel.from_env()
    gbs = config['dataset']['batch_size']
    dcfg = dict(config['dataset'])
    dcfg['batch_size'] = dp.local_batch(gbs)
    if dp.world_size > 1:       # every rank draws the step's grid shape from one shared stream and its samples from its own (dataset._streams)
        dcfg['shard'] = (dp.rank, dp.world_size)
    from .unet import UNetModel
    from .rnn import Dirichlet_BC_RNN
    monitors = ('loss', 'loss')    # what ModelCheckpoint / ReduceLROnPlateau watch
    if args.model in ('dbcnn', 'dbcnn_rnn'):      # train/dbcnn_legacy_train.py:26-31 and train/dbcnn_rnn_train.py:26: one non-zero edge, zero right-hand side
        dataset = numerical_dataset_generator(randomize_boundary_smoothness=True, exclude_zero_boundaries=True, nonzero_boundaries=['left'], rhses='zero',
                                              return_boundaries=True, return_dx=True, return_rhs=False, **dcfg)
        if args.model == 'dbcnn':
            model = Dirichlet_BC_NN_Legacy_2(**config['model'])
        else:                      # train/dbcnn_rnn_train.py:31,38-39: the checkpoint follows 'mse', the learning rate 'loss'
            model = Dirichlet_BC_RNN(**config['model'])
            monitors = ('mse', 'loss')
    elif args.model == 'pcnn':     # train/pcnn_end_to_end.py:28-34: all four edges + a random right-hand side, both sub-models trained jointly
        dataset = numerical_dataset_generator(randomize_boundary_smoothness=True, exclude_zero_boundaries=False, nonzero_boundaries=['left', 'right', 'top', 'bottom'],
                                              rhses='random', return_boundaries=True, return_dx=True, return_rhs=True, **dcfg)
        model = Poisson_CNN_Legacy(Homogeneous_Poisson_NN_Legacy(**config['hpnn_model']), Dirichlet_BC_NN_Legacy_2(**config['dbcnn_model']))
    elif args.model == 'unet':     # train/UNet.py:22-34: dataset by --dataset_type, UNet(**config['model'])
        from .unet import UNet
        dataset = numerical_dataset_generator(**dcfg) if args.dataset_type == 'numerical' else reverse_poisson_dataset_generator(**dcfg)
        model = UNet(**config['model'])
    elif 'model_type' in config['model']:      # train/hpnn_train.py:23-33: the config names the model class; analytic (reverse) dataset
        from .hpnn_models import Homogeneous_Poisson_NN, Homogeneous_Poisson_NN_Metalearning
        mcfg = dict(config['model'])
        model_type = mcfg.pop('model_type')
        classes = {'cnn_metalearning': Homogeneous_Poisson_NN_Metalearning, 'cnn': Homogeneous_Poisson_NN}
        if model_type not in classes:
            raise NotImplementedError('model_type %r (built: %s)' % (model_type, sorted(classes)))
        dataset = reverse_poisson_dataset_generator(**dcfg)
        model = classes[model_type](**mcfg)
    else:
        bc_type = config['model'].get('bc_type', 'dirichlet')
        flags = neumann_flags(bc_type)               # a dict: per-edge boundary types (extension), the numerical generator's mixed Dirichlet/Neumann solve
        if args.dataset_type == 'analytical' and any(flags) and not all(flags):
            raise ValueError('there is no analytic mixed Dirichlet/Neumann generator behind --dataset_type analytical: a per-edge bc_type needs '
                             '--dataset_type analytical_mixed or numerical (got %r)' % (bc_type,))
        neumann = all(flags)
        if args.dataset_type == 'variable_density':        # random smooth rhs and rho, the DST-preconditioned CG solve as ground truth (zero Dirichlet data)
            dataset = variable_density_dataset_generator(**dcfg)
        elif args.dataset_type == 'variable_density_analytical':       # a random series u and rho, rhs = L_h(rho) u from the same launch: no solve
            dataset = reverse_variable_density_dataset_generator(**dcfg)
        elif args.dataset_type == 'analytical_mixed':        # the quarter-wave / whole-wave series of the model's own edge types, homogeneous data
            dataset = reverse_poisson_dataset_generator_mixed(**dict(dcfg, boundary_types=bc_type))
        elif args.dataset_type == 'numerical' and isinstance(bc_type, dict):
            # homogeneous data on every edge (any boundaries string but 'random' is zero data): the mixed solver's ground truth for the model's edge types
            dataset = numerical_dataset_generator(**dict(dcfg, boundary_types=bc_type, boundaries='zero'))
        elif args.dataset_type == 'numerical':
            dataset = numerical_dataset_generator(**dcfg)
        elif neumann:
            dataset = reverse_poisson_dataset_generator_homogeneous_neumann(**dcfg)
        else:
            dataset = reverse_poisson_dataset_generator(**dcfg)
        model = Homogeneous_Poisson_NN_Legacy(**config['model'])
    optimizer = choose_optimizer(config['training']['optimizer'])(**config['training']['optimizer_parameters'])
    if density_model:                                # the flux-form loss with the model's edge types (None: all Dirichlet)
        loss = variable_density_loss_wrapper(global_batch_size=gbs, **dict(config['training']['loss_parameters'], boundary_types=model_bt))
    else:
        loss = loss_wrapper(global_batch_size=gbs, **config['training']['loss_parameters'])
    # the largest batch this run will see, for model.presize(): only where the generator draws its grid shape from a range (the analytic generators)
    rng_ = config['dataset'].get('random_output_shape_range')
    presize = None
    if rng_ is not None and isinstance(model, (Homogeneous_Poisson_NN_Legacy, UNetModel, Dirichlet_BC_RNN)) and os.environ.get('PCNN_PRESIZE', '1') != '0':
        r = np.asarray(rng_, dtype=np.int64)
        r = np.tile(r[None], (2, 1)) if r.ndim == 1 else r
        presize = (dcfg['batch_size'], int(r[0, 1]), int(r[1, 1]))
    model.compile(loss=loss, optimizer=optimizer, max_input_shape=presize)
    dp.attach(model)
    cb = [ModelCheckpoint(args.checkpoint_dir + '/chkpt.checkpoint', monitor=monitors[0]),
          ReduceLROnPlateau(patience=4, monitor=monitors[1], min_lr=config['training']['min_learning_rate']),
          TerminateOnNaN()]
    load_model_checkpoint(model, args.continue_from_checkpoint)
    if args.learning_rate is not None:
        model.optimizer.learning_rate = config['training']['optimizer_parameters']['learning_rate'] if args.learning_rate.lower() == 'from_json' else float(args.learning_rate)
    if dp.rank == 0:
        model.summary()
    model.fit(dataset, epochs=args.epochs or config['training']['n_epochs'], callbacks=cb, verbose=1 if dp.rank == 0 else 0)


if __name__ == '__main__':
    main()
