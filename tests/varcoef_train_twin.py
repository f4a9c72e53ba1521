"""fp64 torch (CPU) twin of the variable-density training operators (poisson_cnn_amd/csrc/varcoef_train.hip).

Fields are (N,H,W) float64 torch tensors (numpy arrays are converted), dx (N,) one spacing per sample.  The discretisation is that of
tests/varcoef_twin.py: beta_face = 2 / (rho_a + rho_b), and
    (L u)[i,j] = sum over the four faces of beta_face (u[neighbour] - u[i,j]) / dx^2 = -(A u)[i,j]      on the (H-2) x (W-2) interior nodes,
with the ring of u part of the field.  Everything here is differentiable by torch.autograd; the hand-written adjoints (residual_loss_grad,
sweep_adjoint) restate what the kernels do - a gather with the symmetric operator - and are checked against autograd in
tests/test_varcoef_train_reference.py."""
import numpy as np
import torch


def t64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device='cpu', dtype=torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def faces(rho):
    """rho (N,H,W) -> the four face coefficients of every interior node, each (N,H-2,W-2): towards i-1, i+1, j-1, j+1."""
    c = rho[:, 1:-1, 1:-1]
    return 2.0 / (c + rho[:, :-2, 1:-1]), 2.0 / (c + rho[:, 2:, 1:-1]), 2.0 / (c + rho[:, 1:-1, :-2]), 2.0 / (c + rho[:, 1:-1, 2:])


def operator(u, rho, dx):
    """L_rho u on the interior nodes, (N,H-2,W-2)."""
    b0, b1, b2, b3 = faces(rho)
    c = u[:, 1:-1, 1:-1]
    s = b0 * (u[:, :-2, 1:-1] - c) + b1 * (u[:, 2:, 1:-1] - c) + b2 * (u[:, 1:-1, :-2] - c) + b3 * (u[:, 1:-1, 2:] - c)
    return s / (dx ** 2)[:, None, None]


def residual(pred, rho, rhs, dx):
    return operator(pred, rho, dx) - rhs[:, 1:-1, 1:-1]


def residual_loss(pred, rho, rhs, dx):
    """(N,) sums over the interior of (L_rho pred - rhs)^2."""
    return (residual(pred, rho, rhs, dx) ** 2).sum(dim=(1, 2))


def _pad(e):
    return torch.nn.functional.pad(e, (1, 1, 1, 1))


def operator_transpose(e, rho, dx):
    """L^T e for e (N,H-2,W-2) -> (N,H,W), as a gather: e extended by zero to all nodes and a one-node halo, then at every node p the sum over
    its faces of beta_face (e[neighbour] - e[p]) / dx^2.  Faces that leave the grid carry e = 0 on both sides."""
    N, H, W = rho.shape
    ez = _pad(_pad(e))                                                   # node (i, j) sits at [i + 1, j + 1]
    rz = torch.nn.functional.pad(rho, (1, 1, 1, 1), value=1.0)
    c, rc = ez[:, 1:-1, 1:-1], rz[:, 1:-1, 1:-1]
    g = (2.0 / (rc + rz[:, :-2, 1:-1]) * (ez[:, :-2, 1:-1] - c) + 2.0 / (rc + rz[:, 2:, 1:-1]) * (ez[:, 2:, 1:-1] - c)
         + 2.0 / (rc + rz[:, 1:-1, :-2]) * (ez[:, 1:-1, :-2] - c) + 2.0 / (rc + rz[:, 1:-1, 2:]) * (ez[:, 1:-1, 2:] - c))
    return g / (dx ** 2)[:, None, None]


def residual_loss_grad(pred, rho, rhs, dx, coef):
    """sum_n coef[n] d(residual_loss[n]) / d(pred), (N,H,W): 2 coef L^T (L pred - rhs)."""
    return 2.0 * coef[:, None, None] * operator_transpose(residual(pred, rho, rhs, dx), rho, dx)


def sweep(u, rho, rhs, dx, n_sweeps=1):
    """n Jacobi sweeps: u' = (sum of beta_face u[neighbour] - dx^2 rhs) / (sum of beta_face) on interior nodes, the ring frozen."""
    b0, b1, b2, b3 = faces(rho)
    d = b0 + b1 + b2 + b3
    f = (dx ** 2)[:, None, None] * rhs[:, 1:-1, 1:-1]
    for _ in range(int(n_sweeps)):
        new = (b0 * u[:, :-2, 1:-1] + b1 * u[:, 2:, 1:-1] + b2 * u[:, 1:-1, :-2] + b3 * u[:, 1:-1, 2:] - f) / d
        u = torch.cat([u[:, :1], torch.cat([u[:, 1:-1, :1], new, u[:, 1:-1, -1:]], dim=2), u[:, -1:]], dim=1)
    return u


def sweep_adjoint(g, rho, dx=None, n_sweeps=1):
    """The transpose of the linear part of `sweep` applied to g (N,H,W): every node receives, from each interior neighbour p, beta_face /
    diagonal(p) times g[p] (written here as p handing it out; the kernel gathers the same terms); a ring node also keeps its own g (it is
    copied through), an interior node does not.  dx does not enter."""
    N, H, W = rho.shape
    b0, b1, b2, b3 = faces(rho)
    d = b0 + b1 + b2 + b3
    ring = torch.ones(H, W, dtype=torch.float64)
    ring[1:-1, 1:-1] = 0.0
    for _ in range(int(n_sweeps)):
        hq = _pad(g[:, 1:-1, 1:-1] / d)                                  # g / diagonal on interior nodes, zero on the ring
        out = ring * g
        out[:, :-2, 1:-1] += b0 * hq[:, 1:-1, 1:-1]                      # interior node p passes to its neighbour towards i-1 ...
        out[:, 2:, 1:-1] += b1 * hq[:, 1:-1, 1:-1]
        out[:, 1:-1, :-2] += b2 * hq[:, 1:-1, 1:-1]
        out[:, 1:-1, 2:] += b3 * hq[:, 1:-1, 1:-1]
        g = out
    return g


def rel_l2(a, b):
    a, b = t64(a).reshape(-1), t64(b).reshape(-1)
    return float((a - b).norm() / b.norm())


# ----------------------------------------------------------------------------- Homogeneous_Poisson_NN_Legacy(density_input=True)
def density_params(cfg, seed, gain=1.6):
    """oracle.hpnn.init_params of the one-channel config, the first kernel widened by a rho slice: [rhs | rho | position channels]."""
    from oracle import hpnn as O
    base = {k: v for k, v in cfg.items() if k != 'density_input'}
    p = O.init_params(base, seed=seed, gain=gain, randomize_all=True)
    k = p['pre/conv0/kernel']                                          # (kh, kw, Cin, Cout)
    rng = np.random.default_rng(seed + 1000)
    lim = O.glorot_limit((k.shape[0], k.shape[1], k.shape[2] + 1, k.shape[3])) * gain
    rho_slice = rng.uniform(-lim, lim, size=k.shape[:2] + (1, k.shape[3])).astype(np.float32).astype(np.float64)
    p['pre/conv0/kernel'] = np.concatenate([k[:, :, :1], rho_slice, k[:, :, 1:]], axis=2)
    return p


def model_forward(ops, cfg, p, stack, dx):
    """oracle.hpnn.forward for the two-channel input, from its public pieces: stack (N,2,H,W) = [rhs, rho], dx (N,1).  Differs from the
    one-channel graph in three places: the input concat, Scaling reading channel 0, and the post-smoother being `sweep` above."""
    from oracle import hpnn as O
    meta, _ = O.build_structure({k: v for k, v in cfg.items() if k != 'density_input'})
    assert meta['bc_type'] == 'dirichlet'
    N, _, H, W = stack.shape
    rhs = stack[:, 0:1]
    x = ops.concat([stack, O.position_embeddings(ops, N, H, W)], 1) if meta['use_pos'] else stack
    dense_inp = ops.concat([dx, dx * (H - 1), dx * (W - 1)], 1)
    pre = meta['pre']
    for i in range(len(pre['layers'])):
        x = ops.padded_conv2d(x, p['pre/conv%d/kernel' % i], p['pre/conv%d/bias' % i], pre['padding_mode'], pre['pad_value'], pre['activation'])
        if meta['use_bn']:
            x = ops.batchnorm_inference(x, *(p['pre/bn%d/%s' % (i, s)] for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')))
    initial = x
    results = [O.bottleneck_forward(ops, p, b, initial, meta['use_bn']) for b in meta['blocks']]
    merged = results[0]
    for r in results[1:]:
        merged = merged + r
    merged = merged / float(len(results) * meta['filters'])
    nb = ops.same_conv2d(initial, p['non_bottleneck_conv/kernel'], p['non_bottleneck_conv/bias'], 'leaky_relu')
    x = ops.same_conv2d(ops.concat([nb, merged], 1), p['post_merge_conv/kernel'], p['post_merge_conv/bias'], 'leaky_relu')
    x = O.resnet_forward(ops, p, 'post_merge_resnet', x, 'constant', 0.0, 'leaky_relu', False)
    d = dense_inp
    for i, act in enumerate(['leaky_relu', 'leaky_relu', 'linear']):
        d = ops.dense(d, p['dx_dense%d/kernel' % i], p['dx_dense%d/bias' % i], act)
    x = x * d[:, :, None, None]
    fin = meta['final']
    for i in range(len(fin['stages'])):
        x = ops.padded_conv2d(x, p['final/stage%d/conv/kernel' % i], p['final/stage%d/conv/bias' % i], fin['padding_mode'], fin['pad_value'], fin['activation'])
        x = O.resnet_forward(ops, p, 'final/stage%d/res' % i, x, 'constant', 0.0, fin['activation'], False)
    for j in range(len(fin['tail'])):
        x = ops.same_conv2d(x, p['final/out%d/kernel' % j], p['final/out%d/bias' % j] if fin['use_bias'] else None, 'linear')
    if meta['use_scaling']:
        x = O.scaling_forward(ops, p, meta['scaling'], x, rhs)
    x = ops.bc_ring(x, 'CONSTANT')
    if meta['postsmoother_iterations'] > 0:
        as_t = isinstance(x, torch.Tensor)
        u = sweep(x[:, 0] if as_t else t64(x[:, 0]), t64(stack[:, 1]), t64(stack[:, 0]), t64(dx).reshape(-1), meta['postsmoother_iterations'])
        x = u[:, None] if as_t else u[:, None].numpy()
    return x


def density_loss(lossp, gbs, y_true, y_pred, stack, dx):
    """variable_density_loss_wrapper in fp64 torch: the oracle's loss_wrapper for the supervised terms (physics-informed weight zeroed) plus
    weight / (N (H-2)(W-2)) * sum of (L_rho pred - rhs)^2, each sample divided by max|rhs|^2 under `normalize`."""
    from oracle import loss as oloss
    base = oloss.loss_wrapper(global_batch_size=gbs, **dict(lossp, physics_informed_loss_weight=0.0))
    N, _, H, W = y_pred.shape
    loss = base(y_true, y_pred, None, None)
    w = float(lossp['physics_informed_loss_weight'])
    if w != 0.0:
        f, rho = t64(stack[:, 0]), t64(stack[:, 1])
        sums = residual_loss(y_pred[:, 0], rho, f, t64(dx).reshape(-1))
        if lossp['physics_informed_loss_config'].get('normalize', False):
            sums = sums / f.abs().amax(dim=(1, 2)) ** 2
        loss = loss + w * sums.sum() / (N * (H - 2) * (W - 2))
    return loss
