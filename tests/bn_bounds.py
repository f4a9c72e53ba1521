"""Training-mode BatchNormalization: test inputs with off-centre channels, the fp64 reference, the error bounds, and a numpy emulation of fp32
accumulation in the kernels' summation order.  Shared by tests/test_gpu_batchnorm.py (the HIP kernels) and tests/test_bn_stats_reference.py (the
emulation: the bounds reject the one-pass sum a, sum a*a formula and admit the centred one).

Bounds (per channel c; u = 2^-24; r_c = |mean_c| / sqrt(var_c + eps) from the fp64 reference).  A kernel that keeps the mean in fp32 and normalises in
fp32 cannot do better than ~u r_c per element in units of the normalised value; four roundings are allowed (the mean, the difference or product,
the scaling, the add):
  y        ||y_c - ref||_2 <= (TOL + 4 u r_c) ||gamma_c xhat_ref,c||_2      (beta and the residual do not enter the scale)
  mean     |d| <= 4 u max(|mean_c|, std_c)
  inv_std  relative TOL_RED on the variance: d(inv_std)/inv_std = 0.5 dvar/(var+eps); plus 4 u for eps in fp32, the add, the root, the division
  scale    inv_std's bound plus one rounding
  moving_mean / moving_variance   the bound of the batch value times (1 - momentum), plus 16 u of that delta because fp32(0.99) makes
           1 - momentum = 0.01 (1 - 9.5e-7), plus 4 u of the stored value (two products, one add, momentum itself)
  dgamma   |d| <= (TOL_RED + 4 u r_c) max(|dgamma_ref|, |sum dy_c|, ||dy_c||_2)
  dbeta    relative TOL_RED
  da       ||d_c||_2 <= (TOL + 4 u r_c) ||da_ref,c||_2
A channel that is exactly constant (or npix = 1) has variance 0: mean = the value and y = beta (+ residual) must then hold exactly in fp32."""
import numpy as np
import torch

from oracle import np_ops, torch_twin

U = 2.0 ** -24
TOL = 2e-6       # tests/test_gpu_ops.py: per-op rel-L2 (fp32 kernels vs fp64 oracle)
TOL_RED = 5e-6   # tests/test_gpu_ops.py: long fp32 reductions
EPS = np_ops.BN_EPS
MOMENTUM = 0.99
RATIOS = (0.0, 3.0, 30.0, 300.0, -100.0)

# (N, H, W, C), channel window of a wider buffer (None: contiguous) - the smallest shape on each route of the sums kernels
SHAPES = {
    'vec4_c28': ((2, 19, 23, 28), None),          # float4 route; C/4 = 7 does not divide the 256-thread block
    'scalar_c6_16k': ((4, 64, 64, 6), None),      # scalar route, C padded to 8; 16384 pixels: many blocks, long per-thread sums
    'npix1': ((1, 1, 1, 8), None),                # one pixel: variance 0, the n/(n-1) guard
    'c256': ((1, 5, 3, 256), None),               # the channel limit; fewer pixels than rows per block
    'c1': ((3, 7, 9, 1), None),
    'slice_aligned': ((2, 9, 11, 8), (16, 4)),    # a[..., 4:12] of a 16-channel buffer: ld = 16, aligned: float4 route
    'slice_misaligned': ((2, 9, 11, 6), (8, 1)),  # a[..., 1:7] of an 8-channel buffer: misaligned base: scalar route
    'ratio0': ((2, 13, 17, 12), None),            # every channel centred, none constant: what the suite exercised before
}


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_case(name):
    """fp32-representable inputs (as fp64, NHWC).  Channel c has offset/sigma = RATIOS[(c + rot) % 5], the sign flipped on every other cycle of 5;
    the last channel (C >= 3) is exactly constant.  'ratio0': all ratios 0, no constant channel."""
    shape, _ = SHAPES[name]
    N, H, W, C = shape
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 100)
    rot = 2 if C == 1 else 0                       # the single channel of the C = 1 case is an off-centre one (ratio 30)
    ratio = np.array([RATIOS[(c + rot) % 5] * (-1.0 if (c // 5) % 2 else 1.0) for c in range(C)]) * (name != 'ratio0')
    sigma = rng.uniform(0.5, 2.0, C)
    a = ratio * sigma + sigma * rng.standard_normal(shape)
    const = np.zeros(C, bool)
    if C >= 3 and name != 'ratio0':
        const[C - 1] = True
        a[..., C - 1] = 1.7
        ratio[C - 1] = np.inf
    if N * H * W == 1:
        const[:] = True
    sign = np.where(np.arange(C) % 3 == 2, -1.0, 1.0)
    d = dict(name=name, a=f32(a), ratio=ratio, const=const,
             gamma=f32(sign * rng.uniform(0.5, 1.5, C)), beta=f32(rng.standard_normal(C)),
             moving_mean=f32(rng.standard_normal(C)), moving_var=f32(rng.uniform(0.5, 2.0, C)),
             residual=f32(rng.standard_normal(shape)),
             # per-channel sum of dy far from 0: the c1 = sum dy / n term of the backward stays live
             dy=f32(rng.standard_normal(shape) + rng.uniform(0.5, 1.0, C) * np.where(np.arange(C) % 2, -1.0, 1.0)))
    return d


def reference(case):
    """fp64: np_ops.batchnorm_training for the values, autograd of torch_twin.batchnorm_training for the gradients."""
    a, gamma, beta = case['a'], case['gamma'], case['beta']
    n = a.size // a.shape[-1]
    y, mean, var = np_ops.batchnorm_training(a.transpose(0, 3, 1, 2), gamma, beta, EPS)
    xt, gt, bt = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (a.transpose(0, 3, 1, 2), gamma, beta))
    yt = torch_twin.batchnorm_training(xt, gt, bt, EPS)[0]
    (yt * torch.tensor(case['dy'].transpose(0, 3, 1, 2))).sum().backward()
    unbias = n / (n - 1.0) if n > 1 else 1.0
    inv_std = 1.0 / np.sqrt(var + EPS)
    return dict(y=y.transpose(0, 2, 3, 1), mean=mean, var=var, inv_std=inv_std, scale=gamma * inv_std, n=n,
                xhat=(a - mean) * inv_std, r=np.abs(mean) * inv_std,
                moving_mean=MOMENTUM * case['moving_mean'] + (1 - MOMENTUM) * mean,
                moving_var=MOMENTUM * case['moving_var'] + (1 - MOMENTUM) * var * unbias, var_delta=(1 - MOMENTUM) * var * unbias,
                da=xt.grad.numpy().transpose(0, 2, 3, 1), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())


def _cnorm(t):
    t = np.asarray(t, np.float64)
    return np.sqrt((t.reshape(-1, t.shape[-1]) ** 2).sum(0))


def forward_checks(case, ref, got, residual=None):
    """{name: (err_c, bound_c)} for got = dict(y, mean, inv_std, scale[, moving_mean, moving_var]) as fp32 arrays."""
    r, const = ref['r'], case['const']
    out = {}
    y_ref = ref['y'] + (residual if residual is not None else 0.0)
    err, bound = _cnorm(got['y'] - y_ref), (TOL + 4 * U * r) * _cnorm(case['gamma'] * ref['xhat'])
    if const.any():       # variance 0: y = beta (+ residual) exactly, as fp32 forms it
        exact = np.float32(case['beta'])[const] + (np.float32(residual)[..., const] if residual is not None else np.float32(0))
        err[const], bound[const] = np.abs(np.asarray(got['y'], np.float64)[..., const] - exact).reshape(-1, const.sum()).max(0), 0.0
    out['y'] = (err, bound)
    out['mean'] = (np.abs(got['mean'] - ref['mean']), np.where(const, 0.0, 4 * U * np.maximum(np.abs(ref['mean']), np.sqrt(ref['var']))))
    is_rel = 0.5 * TOL_RED * ref['var'] / (ref['var'] + EPS) + 4 * U
    out['inv_std'] = (np.abs(got['inv_std'] - ref['inv_std']), ref['inv_std'] * is_rel)
    out['scale'] = (np.abs(got['scale'] - ref['scale']), np.abs(ref['scale']) * (is_rel + U))
    if 'moving_mean' in got:
        out['moving_mean'] = (np.abs(got['moving_mean'] - ref['moving_mean']),
                              (1 - MOMENTUM) * (out['mean'][1] + 16 * U * np.abs(ref['mean'])) + 4 * U * np.abs(ref['moving_mean']))
        out['moving_var'] = (np.abs(got['moving_var'] - ref['moving_var']), (TOL_RED + 16 * U) * ref['var_delta'] + 4 * U * np.abs(ref['moving_var']))
    return out


def backward_checks(case, ref, got):
    """{name: (err_c, bound_c)} for got = dict(da, dgamma, dbeta)."""
    r, dy = ref['r'], case['dy']
    sum_dy = dy.reshape(-1, dy.shape[-1]).sum(0)
    return {
        'dgamma': (np.abs(got['dgamma'] - ref['dgamma']), (TOL_RED + 4 * U * r) * np.maximum.reduce([np.abs(ref['dgamma']), np.abs(sum_dy), _cnorm(dy)])),
        'dbeta': (np.abs(got['dbeta'] - ref['dbeta']), TOL_RED * np.abs(ref['dbeta'])),
        'da': (_cnorm(got['da'] - ref['da']), (TOL + 4 * U * r) * _cnorm(ref['da'])),
    }


def violations(checks):
    """['name[c]: err > bound', ...] - empty when every channel meets every bound."""
    bad = []
    for name, (err, bound) in checks.items():
        for c in np.nonzero(~(err <= bound))[0]:
            bad.append('%s[%d]: %.3g > %.3g' % (name, c, err[c], bound[c]))
    return bad


def worst(checks):
    """{name: max over channels of err / bound} (0/0 counts as 0)."""
    return {name: float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) for name, (err, bound) in checks.items()}


# ---------------------------------------------------------------- fp32 accumulation in the kernels' order, in numpy
def sums_layout(npix, C, vec4):
    """(rows per block R, blocks) of the per-channel sums kernels (csrc/pointwise.hip: colsum_blocks and the two thread layouts)."""
    CP = 1
    while CP < C:
        CP *= 2
    nb = min(1024, max(1, -(-npix // ((256 // CP) * 16))))
    return (256 // (C // 4) if vec4 else 256 // CP), nb


def fp32_colsum(x, R, nb):
    """Column sums of the fp32 array x (npix, C) the way the kernels form them: thread (block b, row q) adds pixels b R + q, + nb R, ... one after the
    other; the block adds its R rows in order; 256 threads add the block partials with stride 256 and a binary tree joins them.  All in fp32."""
    x = np.asarray(x, np.float32)
    npix, C = x.shape
    L = R * nb
    steps = -(-npix // L)
    xp = np.zeros((steps * L, C), np.float32); xp[:npix] = x     # adding +0 is exact
    acc = np.zeros((L, C), np.float32)
    for k in range(steps):
        acc = acc + xp[k * L:(k + 1) * L]
    acc = acc.reshape(nb, R, C)
    part = np.zeros((nb, C), np.float32)
    for q in range(R):
        part = part + acc[:, q]
    pp = np.zeros((-(-nb // 256) * 256, C), np.float32); pp[:nb] = part
    pp = pp.reshape(-1, 256, C)
    t = np.zeros((256, C), np.float32)
    for k in range(pp.shape[0]):
        t = t + pp[k]
    st = 128
    while st > 0:
        t = t[:st] + t[st:2 * st]
        st //= 2
    return t[0]


def emulate(case, scheme, vec4=False):
    """fp32 emulation of forward and backward.  scheme 'naive': sums of a and a*a, var = E[a^2] - E[a]^2, y = a scale + (beta - mean scale),
    dgamma = inv_std (sum dy a - mean sum dy).  scheme 'centred': sums of d = a - K and d*d about K = the tree-added average of the channel's first 8 (4, 2, 1) pixels, mean = K + E[d],
    var = E[d^2] - E[d]^2, y = (a - mean) scale + beta, dgamma = inv_std sum dy (a - mean)."""
    F = np.float32
    C = case['a'].shape[-1]
    a, dy = F(case['a']).reshape(-1, C), F(case['dy']).reshape(-1, C)
    gamma, beta = F(case['gamma']), F(case['beta'])
    n = a.shape[0]
    R, nb = sums_layout(n, C, vec4)
    inv_n, eps = F(1.0 / n), F(EPS)
    if scheme == 'naive':
        m = fp32_colsum(a, R, nb) * inv_n
        v = fp32_colsum(a * a, R, nb) * inv_n - m * m
    else:
        P = 8 if n >= 8 else 4 if n >= 4 else 2 if n >= 2 else 1
        v = np.zeros((8, C), F); v[:P] = a[:P]
        K = (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) * F(1.0 / P)
        d = a - K
        md = fp32_colsum(d, R, nb) * inv_n
        m = K + md
        v = fp32_colsum(d * d, R, nb) * inv_n - md * md
    v = np.maximum(v, F(0))
    inv_std = F(1) / np.sqrt(v + eps)
    scale = gamma * inv_std
    s_dy = fp32_colsum(dy, R, nb)
    if scheme == 'naive':
        y = a * scale + (beta - m * gamma * inv_std)
        dg = inv_std * (fp32_colsum(dy * a, R, nb) - m * s_dy)
    else:
        y = (a - m) * scale + beta
        dg = inv_std * fp32_colsum(dy * (a - m), R, nb)
    c1, c2 = s_dy * inv_n, dg * inv_n
    da = scale * (dy - c1 - (a - m) * inv_std * c2)
    assert all(t.dtype == np.float32 for t in (m, v, inv_std, scale, y, dg, da))
    shape = case['a'].shape
    return dict(y=y.reshape(shape), mean=m, var=v, inv_std=inv_std, scale=scale, da=da.reshape(shape), dgamma=dg, dbeta=s_dy)
