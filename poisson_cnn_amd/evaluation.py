"""Host side of model.evaluate() / predict(): cutting inputs into batches and turning the per-sample rows of ops.error_stats into the
figures evaluate() returns.  Pure numpy in float64 - nothing here touches the GPU, so tests/test_error_stats_host.py runs it without one.

One batch contributes a vector of SUMS (`batch_totals`) and one maximum; vectors add over batches and - under data parallelism - over ranks
(parallel.DataParallel.global_eval_totals: one all-reduce(SUM) of the vector, one all-reduce(MAX) of the maximum), and `finish` divides."""
import numpy as np

# the columns of ops.error_stats
SUM_ABS_E, SUM_E2, MAX_ABS_E, SUM_T2, MAX_ABS_T, SUM_R2, MAX_ABS_R, SUM_F2 = range(8)

TOTALS = ('loss_n', 'n', 'sum_e2', 'sum_abs_e', 'sum_hw', 'sum_rel_l2', 'sum_mae_over_peak', 'n_rel_l2', 'sum_rel_residual', 'n_rel_residual')
_UNSUPPORTED = ('sample_weight', 'class_weight', 'validation_split')


def reject_unsupported(who, kwargs):
    """The Keras arguments that would change the result and are not implemented raise NotImplementedError; anything else is an unknown keyword."""
    for k in kwargs:
        if k in _UNSUPPORTED:
            raise NotImplementedError('%s: %s is not implemented' % (who, k))
        raise TypeError('%s() got an unexpected keyword argument %r' % (who, k))


def is_sequence(x):
    """A Keras-Sequence-style dataset (`__len__`, `__getitem__` -> (inputs, target)) as opposed to an input list."""
    return hasattr(x, '__len__') and hasattr(x, '__getitem__') and not isinstance(x, (list, tuple, dict)) and not hasattr(x, 'shape')


class ArrayBatches:
    """An input list (and optional targets) cut into chunks of `batch_size` samples along axis 0, with the Sequence interface.  Entries of the
    input list that are not arrays over the samples (the boundary models' x_output_resolution) go into every chunk as they are."""

    def __init__(self, inputs, y=None, batch_size=None):
        self.inputs, self.y = list(inputs), y
        sized = [v for v in self.inputs if hasattr(v, 'shape') and len(v.shape) >= 1]
        if not sized:
            raise ValueError('the input list holds no array')
        self.n = int(sized[0].shape[0])
        for v in sized + ([y] if y is not None else []):
            if int(v.shape[0]) != self.n:
                raise ValueError('inputs and targets disagree on the number of samples: %d vs %d' % (int(v.shape[0]), self.n))
        self.batch_size = 32 if batch_size is None else int(batch_size)              # Keras' default
        if self.batch_size < 1:
            raise ValueError('batch_size must be >= 1')

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        a, b = i * self.batch_size, min((i + 1) * self.batch_size, self.n)
        inp = [v[a:b] if hasattr(v, 'shape') and len(v.shape) >= 1 else v for v in self.inputs]
        return inp, (None if self.y is None else self.y[a:b])


def batch_totals(stats, H, W, loss, global_batch_size=None):
    """One batch -> (the TOTALS vector, max|e|).  stats: the (n, 8) rows of ops.error_stats; loss: the compiled loss of the batch, which is a
    sum over its samples divided by `global_batch_size` (the batch's own size when None), so loss * that size is the batch's sum of per-sample
    losses.  Samples whose target (right-hand side) is identically zero have no relative error (residual): they stay out of that mean and
    of its count."""
    s = np.asarray(stats, dtype=np.float64).reshape(-1, 8)
    n, hw = s.shape[0], float(H) * float(W)
    ok_t, ok_f = s[:, SUM_T2] > 0.0, s[:, SUM_F2] > 0.0
    rel_l2 = np.sqrt(s[ok_t, SUM_E2] / s[ok_t, SUM_T2])
    mae_peak = (s[ok_t, SUM_ABS_E] / hw) / s[ok_t, MAX_ABS_T]
    rel_res = np.sqrt(s[ok_f, SUM_R2] / s[ok_f, SUM_F2])
    gbs = n if global_batch_size is None else int(global_batch_size)
    tot = np.array([float(loss) * gbs, n, s[:, SUM_E2].sum(), s[:, SUM_ABS_E].sum(), n * hw, rel_l2.sum(), mae_peak.sum(), ok_t.sum(),
                    rel_res.sum(), ok_f.sum()], dtype=np.float64)
    return tot, (float(s[:, MAX_ABS_E].max()) if n else 0.0)


def finish(totals, max_abs_error):
    """The summed TOTALS vector and the overall maximum -> evaluate()'s dict.  A mean over no samples (every target zero; a model without a
    right-hand side among its inputs, for which the residual columns are all zero) is NaN."""
    t = dict(zip(TOTALS, np.asarray(totals, dtype=np.float64)))

    def div(a, b):
        return float(a / b) if b > 0 else float('nan')
    return {'loss': div(t['loss_n'], t['n']), 'mse': div(t['sum_e2'], t['sum_hw']), 'mae': div(t['sum_abs_e'], t['sum_hw']),
            'rel_l2': div(t['sum_rel_l2'], t['n_rel_l2']), 'mae_over_peak': div(t['sum_mae_over_peak'], t['n_rel_l2']),
            'max_abs_error': float(max_abs_error), 'rel_residual': div(t['sum_rel_residual'], t['n_rel_residual']),
            'skipped_rel_l2': int(round(t['n'] - t['n_rel_l2'])), 'skipped_rel_residual': int(round(t['n'] - t['n_rel_residual'])),
            'samples': int(round(t['n']))}
