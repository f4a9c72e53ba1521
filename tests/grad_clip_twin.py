"""Gradient clipping and learning-rate decay of tf.keras OptimizerV2 (TF 2.4) restated in fp64 numpy, the synthetic bucket the tests share, and
the error bound of the library's two-stage fp32 sum of squares.  Shared by tests/test_grad_clip_host.py and tests/test_gpu_grad_clip.py.

Semantics (OptimizerV2._clip_gradients; tf.clip_by_norm, tf.clip_by_global_norm, tf.clip_by_value), g = grad_scale * gradient:
  clipnorm c          g_v <- g_v c / max(||g_v||_2, c) per variable           (norm <= c: scale exactly 1)
  global_clipnorm c   G = sqrt(sum_v ||g_v||^2) over all variables of all buckets; g <- g c / max(G, c); G not finite: every g is NaN
  clipvalue c         g <- min(max(g, -c), c), after either norm clip
  decay d             the step uses lr / (1 + d t), t = number of updates already applied

Bound of the squared norm of one variable (u = 2^-24; csrc/grad_clip.hip states the order of the sum).  Every term fl(fl(s g)^2) carries three
roundings (the product s g, the square, and - counted here - the term's first addition); all terms are >= 0, so a sum through k fp32 additions
has relative error <= gamma_k = k u / (1 - k u).  An item of L floats is added through at most
    lane:  4 ceil(floor(L / 4) / 256) + 2      (the float4 rounds of a lane, component by component, plus a head and a tail float)
    wave:  6                                    (butterfly over 64 lanes)
    LDS:   2                                    ((w0 + w1) + (w2 + w3))
additions.  The variable's items are then added in a double (n_items roundings of 2^-53), the fp64 reference itself sums n terms (n 2^-53), and the
stored squared norm is rounded to fp32 once (u).  No term may underflow: the test data keeps |s g| > 1e-15."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
CHUNK = 4096           # PCNN_GRAD_CLIP_CHUNK
THREADS = 256
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099]
ZERO_VAR, SMALL_VAR, AT_C_VAR, BIG_VAR = 3, 5, 8, 10       # all zero / norm far below c / norm == c within rounding / norm far above c


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def make_bucket(c=1.0, seed=0, sizes=SIZES):
    """list of fp32 arrays, one per variable: random normal (norm ~ sqrt(size)), except the four marked variables."""
    rng = np.random.default_rng(seed)
    g = [rng.standard_normal(n) for n in sizes]
    if sizes is SIZES:
        g[ZERO_VAR][:] = 0.0
        g[SMALL_VAR] *= 1e-3 * c / np.linalg.norm(g[SMALL_VAR])
        g[AT_C_VAR] *= c / np.linalg.norm(g[AT_C_VAR])
        g[BIG_VAR] *= 100.0 * c
    return [f32(v) for v in g]


def split(flat, sizes=SIZES):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [np.asarray(flat)[off[i]:off[i + 1]] for i in range(len(sizes))]


def sqnorms(gvars, grad_scale=1.0):
    """fp64 ||grad_scale g_v||^2 per variable (grad_scale as the fp32 value the library receives)."""
    s = float(np.float32(grad_scale))
    return np.array([np.sum((s * np.asarray(v, np.float64)) ** 2) for v in gvars])


def global_norm(buckets, grad_scale=1.0):
    return float(np.sqrt(sum(sqnorms(b, grad_scale).sum() for b in buckets)))


def clip(buckets, grad_scale=1.0, clipnorm=None, global_clipnorm=None, clipvalue=None, variant='tf'):
    """buckets: list of buckets, each a list of per-variable arrays -> the clipped gradients in fp64, same nesting.
    variant 'tf': the semantics above.  Two deliberately WRONG variants, which the tests must be able to tell from it:
    'global_for_per_variable' (clipnorm scales by the global norm) and 'clipvalue_first' (the clamp in front of the norm clip)."""
    assert clipnorm is None or global_clipnorm is None
    s = float(np.float32(grad_scale))
    out = [[s * np.asarray(v, np.float64) for v in b] for b in buckets]

    def clamp(bs):
        if clipvalue is None:
            return bs
        cv = float(np.float32(clipvalue))
        return [[np.minimum(np.maximum(v, -cv), cv) for v in b] for b in bs]      # numpy propagates NaN, as tf.clip_by_value does

    def norm_clip(bs):
        if clipnorm is not None and variant != 'global_for_per_variable':
            c = float(np.float32(clipnorm))
            return [[v * (c / max(np.sqrt(np.sum(v * v)), c)) if np.isfinite(np.sum(v * v)) else v * np.nan for v in b] for b in bs]
        c = clipnorm if clipnorm is not None else global_clipnorm
        if c is None:
            return bs
        c = float(np.float32(c))
        G = np.sqrt(sum(np.sum(v * v) for b in bs for v in b))
        scale = c / max(G, c) if np.isfinite(G) else np.nan
        return [[v * scale for v in b] for b in bs]

    return norm_clip(clamp(out)) if variant == 'clipvalue_first' else clamp(norm_clip(out))


def scales(gvars, c, grad_scale=1.0):
    """fp64 per-variable clipnorm scales c / max(||g_v||, c)."""
    c = float(np.float32(c))
    return c / np.maximum(np.sqrt(sqnorms(gvars, grad_scale)), c)


def decayed_lr(lr, decay, t):
    return lr / (1.0 + decay * t)


# ---------------------------------------------------------------- the bound
def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def item_lengths(size, chunk=CHUNK):
    return [min(chunk, size - s) for s in range(0, size, chunk)]


def sqnorm_rel_bound(size, chunk=CHUNK, threads=THREADS):
    """Relative error bound of the library's squared norm of a variable of `size` floats against the fp64 reference (derivation: module docstring)."""
    lens = item_lengths(size, chunk)
    if not lens:
        return 0.0
    adds = max(4 * -(-(L // 4) // threads) + 2 for L in lens) + 6 + 2
    fp32_part = gamma(adds + 2)                                   # + the product s g and the square
    return (1 + fp32_part) * (1 + gamma(len(lens), U64)) * (1 + gamma(size, U64)) * (1 + U) - 1


def total_rel_bound(sizes, chunk=CHUNK):
    """... of a sum of squared norms over variables (double additions, one more per variable; the result is read as a double or rounded to fp32 once)."""
    return (1 + max(sqnorm_rel_bound(n, chunk) for n in sizes)) * (1 + gamma(len(sizes), U64)) * (1 + U) - 1


def scale_rel_bound(sq_rel):
    """c / sqrt(S) for S within sq_rel of the truth: d(scale) / scale <= 1 / sqrt(1 - sq_rel) - 1; the library forms the quotient in double (two
    roundings of 2^-53) and rounds it to fp32 once."""
    return (1.0 / np.sqrt(1.0 - sq_rel)) * (1 + 2 * U64) * (1 + U) - 1
