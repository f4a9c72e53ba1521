"""Float64 NumPy formulas of the entry points that only pipelines reach (include/pcnn.h): the fp64 batched GEMM, series synthesis, separable sums, strided
sub-sampling and its adjoint, the input assemblies with their positional channels, the first-row overwrite, flip / rotate, the boundary expansion and its
adjoint, and the per-sample / per-channel scalings - one function per operation, straight from the formula in each kernel's header comment - together with
the cases, the inputs and the bounds that tests/test_entry_points_reference.py (CPU) and tests/test_gpu_entry_points.py (GPU) share.

Every function computes in the precision of its arguments: called on float32 arrays it is the float32 evaluation the bounds are measured against.

Bounds.  Copies and index maps are exact.  The GEMM is exact on small integers and within gemm_bound on normals.  One-rounding element-wise operations
take TOL of tests/test_gpu_ops.py.  Where another test of the same op has a bound it is the floor here (2e-6 for series synthesis and separable sums in
tests/test_gpu_dataset.py, 1e-6 / 2e-6 for the boundary expansion in tests/test_gpu_dbcnn.py); every wider bound is 4 x the error of the SAME function below
evaluated in float32 by NumPy on the CPU on the test's own inputs (4 x because the order of the sums differs), and the measured figures stand beside
the bounds.  The CPU test re-measures every figure and asserts it under its bound."""
import functools
import zlib

import numpy as np

TOL = 2e-6                      # per-op rel-L2 (fp32 kernels vs fp64), as in tests/test_gpu_ops.py
GRID_CAP = 8192 * 256           # threads of the capped grid of csrc/pointwise.hip (grid1d)
DATASET_CAP = 16384 * 256       # ... of csrc/dataset.hip and csrc/dbcnn.hip


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def rng_of(*key):
    """One generator per case, the same in both test files."""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bound_of(floor, table, key):
    return max(floor, 4 * table.get(key, 0.0))


# ----------------------------------------------------------------------------- 1. fp64 batched GEMM, C[b] = A[b] B[b]
GEMM_SHAPES = [(1, 1, 1), (16, 16, 4), (64, 64, 16), (65, 63, 17), (33, 130, 70), (130, 33, 5), (129, 129, 3)]
GEMM_FORMS = ['single', 'shared_a', 'shared_b']     # batch 1; batch 3 with strideA = 0; batch 3 with strideB = 0
GEMM_KINDS = ['int', 'normal']
GEMM_PADDED = (65, 63, 17)                          # run once more with lda, ldb, ldc 3 past the row


def gemm(A, B):
    """A (batch or 1, M, K), B (batch or 1, K, N) -> (batch, M, N); a leading 1 is the stride-0 broadcast."""
    return np.matmul(A, B)


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, form, kind):
    """'int': integers of [-8, 8] as doubles - every product and partial sum is an exact double in any order.  'normal': standard normals."""
    rng = rng_of('gemm', M, N, K, form, kind)
    batch = 1 if form == 'single' else 3
    sa, sb = (1 if form == 'shared_a' else batch, M, K), (1 if form == 'shared_b' else batch, K, N)
    draw = (lambda s: rng.integers(-8, 9, s).astype(np.float64)) if kind == 'int' else rng.standard_normal
    A, B = draw(sa), draw(sb)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def gemm_bound(A, B):
    """|C - C_ref| <= 2 K 2^-53 (|A| |B|) element-wise: the dot-product bound of any summation order, once for the kernel and once for the reference."""
    return 2 * A.shape[-1] * 2.0 ** -53 * np.matmul(np.abs(A), np.abs(B))


# ----------------------------------------------------------------------------- 2. series synthesis
SERIES_MODES = [(1, 1), (16, 16), (3, 16), (16, 2)]
SERIES_SHAPES = [(1, 255), (15, 255), (16, 255), (17, 255), (33, 255), (17, 1), (17, 256), (17, 257), (1, 1)]     # every H at W = 255, every W at H = 17, the corner
SERIES_ACC_SHAPES = [(17, 257), (1, 1)]             # accumulate=True onto a random base
SERIES_WIDEST = (17, 1008)                          # ka = 16: (16 x 1008 + 16 x 16) floats = 64 KiB of LDS exactly; W = 1009 is refused
SERIES_TOL = 2e-6                                   # tests/test_gpu_dataset.py, 5 x 8 modes
# rel-L2 of series() in float32 against float64 on series_inputs, (ka, kb, trig, H, W) -> figure, wherever it is above SERIES_TOL / 4: the arguments reach
# 16 pi in float32, where half an ulp is 1.9e-6
SERIES_MEASURED = {
    (16, 16, 0, 15, 255): 1.05e-06, (16, 16, 0, 16, 255): 1.02e-06, (16, 16, 0, 17, 255): 9.59e-07, (16, 16, 0, 33, 255): 9.01e-07,
    (16, 16, 0, 17, 256): 9.54e-07, (16, 16, 0, 17, 257): 9.45e-07, (16, 16, 0, 17, 1008): 9.50e-07,
    (16, 16, 1, 1, 255): 5.60e-07, (16, 16, 1, 15, 255): 8.39e-07, (16, 16, 1, 16, 255): 8.11e-07, (16, 16, 1, 17, 255): 8.14e-07,
    (16, 16, 1, 33, 255): 8.57e-07, (16, 16, 1, 17, 256): 8.12e-07, (16, 16, 1, 17, 257): 8.09e-07, (16, 16, 1, 17, 1008): 8.18e-07,
    (3, 16, 0, 15, 255): 6.58e-07, (3, 16, 0, 16, 255): 6.49e-07, (3, 16, 0, 17, 255): 6.42e-07, (3, 16, 0, 33, 255): 6.49e-07,
    (3, 16, 0, 17, 256): 6.55e-07, (3, 16, 0, 17, 257): 6.45e-07,
    (3, 16, 1, 1, 255): 6.42e-07, (3, 16, 1, 15, 255): 6.59e-07, (3, 16, 1, 16, 255): 6.53e-07, (3, 16, 1, 17, 255): 6.50e-07,
    (3, 16, 1, 33, 255): 6.53e-07, (3, 16, 1, 17, 256): 6.46e-07, (3, 16, 1, 17, 257): 6.15e-07,
    (16, 2, 0, 15, 255): 8.29e-07, (16, 2, 0, 16, 255): 9.14e-07, (16, 2, 0, 17, 255): 6.32e-07, (16, 2, 0, 33, 255): 7.23e-07,
    (16, 2, 0, 17, 256): 6.31e-07, (16, 2, 0, 17, 257): 6.30e-07, (16, 2, 0, 17, 1008): 6.31e-07,
    (16, 2, 1, 15, 255): 6.12e-07, (16, 2, 1, 16, 255): 5.81e-07, (16, 2, 1, 17, 255): 6.47e-07, (16, 2, 1, 33, 255): 6.83e-07,
    (16, 2, 1, 17, 1): 7.20e-07, (16, 2, 1, 17, 256): 6.47e-07, (16, 2, 1, 17, 257): 6.47e-07, (16, 2, 1, 17, 1008): 6.47e-07,
}


def _series(coef, H, W, trig, over_n=False, first_mode=1, swap=False):
    dt = coef.dtype
    _, ka, kb = coef.shape
    f = (np.cos if trig else np.sin) if not swap else (np.sin if trig else np.cos)
    grid = lambda n: (np.arange(n) * (np.pi / n) if over_n else np.linspace(0, np.pi, n)).astype(dt)
    Fa = f(np.outer(grid(H), np.arange(first_mode, first_mode + ka).astype(dt)))
    Fb = f(np.outer(grid(W), np.arange(first_mode, first_mode + kb).astype(dt)))
    return np.einsum('aA,nAb->nab', Fa, np.einsum('nAB,bB->nAb', coef, Fb))


def series(coef, H, W, trig, base=None):
    """coef (N, ka, kb) -> (N, H, W): sum c[A,B] f((A+1) x_a) f((B+1) y_b) on x = linspace(0, pi, H), y = linspace(0, pi, W); f = sin (trig 0) / cos (trig 1)."""
    out = _series(coef, H, W, trig)
    return out if base is None else base + out


@functools.lru_cache(maxsize=None)
def series_inputs(ka, kb):
    return f32(rng_of('series', ka, kb).uniform(-1, 1, (2, ka, kb)))


@functools.lru_cache(maxsize=None)
def series_base(H, W):
    return f32(rng_of('series base', H, W).standard_normal((2, H, W)))


# ----------------------------------------------------------------------------- 3. separable sums, per-sample scaling, max-magnitude normalisation
SEPSUM_SHAPES = [(3, 9, 14), (2, 1, 5)]
SEPSUM_RANKS = [1, 2, 7]
SEPSUM_TOL = 2e-6                                   # tests/test_gpu_dataset.py, R = 2
BIG_FIELD, BIG_RANK = (2, 1100, 2000), 2            # 4 400 000 elements > DATASET_CAP
# float32 on the CPU: separable_sum() <= 6.2e-8 over every case, the base included: below SEPSUM_TOL / 4, so SEPSUM_TOL holds


def separable_sum(U, V, base=None):
    """U (N, R, H), V (N, R, W) -> (N, H, W): einsum('nra,nrb->nab')."""
    out = np.einsum('nra,nrb->nab', U, V)
    return out if base is None else base + out


@functools.lru_cache(maxsize=None)
def sepsum_inputs(N, H, W, R):
    rng = rng_of('sepsum', N, H, W, R)
    return f32(rng.standard_normal((N, R, H))), f32(rng.standard_normal((N, R, W))), f32(rng.standard_normal((N, H, W)))


def scale_samples(x, s):
    return x * s.reshape((-1,) + (1,) * (x.ndim - 1))


def set_max_magnitude(x, target):
    """-> (x[n] target[n] / max|x[n]|, the factors)."""
    fac = target / np.abs(x).reshape(x.shape[0], -1).max(1)
    return scale_samples(x, fac), fac


@functools.lru_cache(maxsize=None)
def field_inputs(shape):
    """A field with a sample axis, one scale per sample."""
    rng = rng_of('field', shape)
    return f32(rng.standard_normal(shape)), f32(rng.uniform(0.5, 2.0, shape[0]) * np.where(np.arange(shape[0]) % 2, -1.0, 1.0))


# ----------------------------------------------------------------------------- 4. strided sub-sampling and its adjoint
SUB_STRIDES = [1, 2, 3, 4]
SUB_GRIDS = [(21, 26), (1, 1), (5, 1), (4, 9)]
SUB_CHANNELS = [1, 5, 8]
SUB_BIG, SUB_BIG_STRIDE = (2, 2060, 2047, 1), 2     # 2 x 1030 x 1024 = 2 109 440 coarse elements > GRID_CAP, so both directions wrap


def subsample(x, s):
    """(N, H, W, C) -> x[:, ::s, ::s, :]."""
    return x[:, ::s, ::s, :]


def subsample_bwd(dy, full_hw, s):
    """The adjoint: dy scattered into zeros of (N, H, W, C)."""
    dx = np.zeros((dy.shape[0],) + tuple(full_hw) + (dy.shape[3],), dy.dtype)
    dx[:, ::s, ::s, :] = dy
    return dx


@functools.lru_cache(maxsize=None)
def sub_inputs(H, W, C, s, N=2):
    """x (N, H, W, C) and a coarse gradient dy; no two elements of either are equal, so a copy from the wrong place cannot pass."""
    rng = rng_of('sub', H, W, C, s, N)
    Ho, Wo = -(-H // s), -(-W // s)
    x = f32(rng.permutation(N * H * W * C).reshape(N, H, W, C) + 1.0)
    dy = f32(-(rng.permutation(N * Ho * Wo * C).reshape(N, Ho, Wo, C) + 1.0))
    return x, dy


# ----------------------------------------------------------------------------- 5. input assembly and the positional channels
ASM_GRIDS = [(33, 47), (7, 1), (1, 9), (1, 1), (2, 2)]
ASM_BIG = (3, 840, 841)                             # 2 119 320 pixels > GRID_CAP
DBC_LENGTHS = [1, 2, 61]
COS_TOL = 1e-6      # max-abs of a cosine channel (the reference is O(1)): tests/test_gpu_dbcnn.py's figure.  Format reasoning gives the same: the argument
                    # pi t carries four float32 roundings (pi, 1 / (n - 1), the two products), 2.1e-7 relative on at most pi, and cosf an ulp or two: 8e-7
# float32 on the CPU: cos_channel(n) is off by at most 2.3e-7 (n = 841) over every axis length the tests use: below COS_TOL / 4, so COS_TOL holds


def linspace01(n, dt=np.float64):
    """tf.linspace(0, 1, n); linspace(0, 1, 1) = [0]."""
    return np.linspace(0.0, 1.0, n).astype(dt)


def cos_channel(n, dt=np.float64):
    """cos(pi linspace(0, 1, n)) in the precision dt."""
    return np.cos(np.dtype(dt).type(np.pi) * linspace01(n, dt))


def _pos_channels(N, H, W, dt):
    return np.broadcast_to(cos_channel(H, dt)[None, :, None], (N, H, W)), np.broadcast_to(cos_channel(W, dt)[None, None, :], (N, H, W))


def assemble_input(rhs, use_pos=True):
    """rhs (N, H, W) -> (N, H, W, 3 or 1): [rhs | cos(pi y) | cos(pi x)]."""
    return np.stack((rhs,) + (_pos_channels(*rhs.shape, rhs.dtype) if use_pos else ()), -1)


def assemble_density_input(stack, use_pos=True):
    """stack (N, 2, H, W) = [rhs, rho] -> (N, H, W, 4 or 2): [rhs | rho | cos(pi y) | cos(pi x)]."""
    N, _, H, W = stack.shape
    return np.stack((stack[:, 0], stack[:, 1]) + (_pos_channels(N, H, W, stack.dtype) if use_pos else ()), -1)


def dbc_assemble_input(bc):
    """bc (N, L) -> (N, 1, L, 3): [bc | 1 | cos(pi y)]."""
    N, L = bc.shape
    return np.stack((bc, np.ones_like(bc), np.broadcast_to(cos_channel(L, bc.dtype), (N, L))), -1)[:, None]


@functools.lru_cache(maxsize=None)
def asm_inputs(N, H, W):
    """(N, 2, H, W): channel 0 is the rhs of assemble_input, the pair the stack of assemble_density_input."""
    return f32(rng_of('asm', N, H, W).standard_normal((N, 2, H, W)))


@functools.lru_cache(maxsize=None)
def bc_inputs(N, L):
    return f32(rng_of('bc', N, L).standard_normal((N, L)))


# ----------------------------------------------------------------------------- 6. first-row overwrite
FIRST_ROW_SHAPES = [(3, 5, 7), (2, 1, 4), (2, 6, 1)]


def set_first_row(y, bc=None):
    """y (N, X, L) with y[:, 0, :] = bc (N, L), or zeros."""
    out = y.copy()
    out[:, 0, :] = 0.0 if bc is None else bc
    return out


# ----------------------------------------------------------------------------- 7. flip / rotate
FLIP_SHAPES = [(3, 7, 5), (2, 1, 6)]
FLIP_COMBOS = [(t, fy, fx) for t in (False, True) for fy in (False, True) for fx in (False, True)]
FLIP_BIG, FLIP_BIG_COMBO = (2, 1449, 1448), (True, True, False)      # 4 196 304 elements > DATASET_CAP


def flip_rotate(x, transpose, flip_y, flip_x, alpha=None, base=None):
    """x (N, H, W) -> reverse(transpose?(x)) along the flagged axes of the OUTPUT, times alpha[n], plus base."""
    out = x.transpose(0, 2, 1) if transpose else x
    out = out[:, ::-1] if flip_y else out
    out = out[:, :, ::-1] if flip_x else out
    out = out if alpha is None else alpha[:, None, None] * out
    return np.ascontiguousarray(out) if base is None else base + out


@functools.lru_cache(maxsize=None)
def flip_inputs(shape):
    """x, alpha (N,), a base of the transposed and one of the untransposed output shape."""
    rng = rng_of('flip', shape)
    N, H, W = shape
    return (f32(rng.standard_normal(shape)), f32(rng.uniform(0.5, 2.0, N) * np.where(np.arange(N) % 2, -1.0, 1.0)), f32(rng.standard_normal((N, W, H))),
            f32(rng.standard_normal(shape)))


# ----------------------------------------------------------------------------- 8. boundary expansion einsum('bmy,mx,bm->bmxy') and its adjoint
DBC_EXPAND_SHAPES = [(2, 9, 13, 5), (3, 1, 4, 1), (2, 6, 1, 3), (3, 4, 5, 32)]     # (N, X, L, M); N M = 96 > 64 is a second block of the dense kernel
DBC_FWD_TOL, DBC_BWD_TOL = 1e-6, 2e-6               # tests/test_gpu_dbcnn.py
# float32 on the CPU: the product channels <= 4.9e-8, df <= 7.6e-8, dd <= 1.1e-7 over the four shapes: below a quarter of each floor, so the floors hold


def dbc_expand(f, sh, d):
    """f (N, 1, L, M), sh (M, X), d (N, M) -> (N, X, L, M + 2): out[n,x,y,m] = f[n,y,m] sh[m,x] d[n,m], then cos(pi x / (X-1)) and cos(pi y / (L-1))."""
    N, _, L, M = f.shape
    X = sh.shape[1]
    ex, ey = _pos_channels(N, X, L, f.dtype)
    return np.concatenate([np.einsum('nym,mx,nm->nxym', f[:, 0], sh, d), ex[..., None], ey[..., None]], -1)


def dbc_expand_bwd(dout, f, sh, d):
    """dout (N, X, L, >= M) -> (df (N, 1, L, M), dd (N, M)) of sum(dout[..., :M] * dbc_expand(f, sh, d)[..., :M])."""
    M = f.shape[3]
    t = np.einsum('nxym,mx->nym', dout[..., :M], sh)
    return (t * d[:, None, :])[:, None], np.einsum('nym,nym->nm', t, f[:, 0])


@functools.lru_cache(maxsize=None)
def dbc_inputs(N, X, L, M):
    """f, sh, d and a gradient dout (N, X, L, M + 2).  sh is random, not the model's sinh table: it has no symmetry in m or x."""
    rng = rng_of('dbc', N, X, L, M)
    return f32(rng.standard_normal((N, 1, L, M))), f32(rng.uniform(-1, 1, (M, X))), f32(rng.standard_normal((N, M))), f32(rng.standard_normal((N, X, L, M + 2)))


# ----------------------------------------------------------------------------- 9. per-channel and per-sample scaling
SCALE_CHANNELS = [1, 3, 32]
SCALE_GRID = (9, 10)
SCALE_BIG = (3, 500, 500, 3)                        # 2 250 000 elements > GRID_CAP


def channel_scale(x, s):
    """x (N, H, W, C), s (N, C) -> x s[n, c]."""
    return x * s[:, None, None, :]


def sample_scale(x, g):
    """x (N, ...), g (N,) -> x (1 + g[n])."""
    return x * (1 + g).reshape((-1,) + (1,) * (x.ndim - 1))


@functools.lru_cache(maxsize=None)
def scale_inputs(shape):
    rng = rng_of('scale', shape)
    return f32(rng.standard_normal(shape)), f32(rng.standard_normal((shape[0], shape[3]))), f32(rng.standard_normal(shape[0]))
