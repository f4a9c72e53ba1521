"""torch CPU twin of the variable-density Jacobi smoother's gradients with respect to u, rho and rhs (pcnn_varcoef_bc_jacobi_bwd_inputs of
poisson_cnn_amd/csrc/varcoef_train.hip, autograd.variable_density_smooth), in the notation of tests/varcoef_bc_twin.py.

One sample: fields (H,W), spacing dx, mask bit 0/1/2/3 = left / right / bottom / top (rows 0 / H-1, columns 0 / W-1) is Neumann with du/dn = 0.
Two independent routes to every gradient:
  * `sweep` is the smoother written with plain differentiable torch ops - every node reads its four neighbours through index lists that mirror at the
    ends of an axis, which counts the inward face of a Neumann edge node twice, and the Dirichlet nodes copy through - and `autograd_grads` lets
    torch.autograd differentiate n sweeps of it;
  * `closed_form` is the hand-written backward the kernel implements, face by face on whole-array slices: per sweep u -> u', walking backwards, with
    g' = d loss / d u', D_c = sum_k m_k beta_k, a_c = g'_c / D_c on the unknowns and 0 on every other node,
        du_k    = sum over the unknown neighbours c of k of m beta a_c  (+ g'_k on a frozen node)
        drhs_c += -h^2 a_c
        drho_p += sum over the faces (c, k) that touch p, c an unknown, of -1/2 beta^2 m a_c (u_k - u'_c)
    (beta = 2 / (rho_a + rho_b), m = 2 where c has no neighbour on its other side - a Neumann edge node).  It takes any float dtype: run in float32
    it is the floor of an fp32 evaluation of the same formulas."""
import functools

import numpy as np
import torch

from tests import varcoef_bc_twin as B

KEYS = ('u', 'rho', 'rhs')


def _t(a, dtype=torch.float64):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=dtype)


def unknown_mask(H, W, mask):
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    m = torch.zeros((H, W), dtype=torch.bool)
    m[i0:i1 + 1, j0:j1 + 1] = True
    return m


def _mirrored(n):
    """The indices of the neighbours towards -1 and +1 of each entry of an n-long axis; the ends read their inward neighbour."""
    lo, hi = torch.arange(n) - 1, torch.arange(n) + 1
    lo[0], hi[-1] = 1, n - 2
    return lo, hi


def sweep_once(u, rho, rhs, dx, mask):
    """One sweep, differentiable in u, rho and rhs (tensors of one dtype)."""
    H, W = u.shape
    h2 = torch.tensor(float(dx), dtype=u.dtype) ** 2
    (up, down), (left, right) = _mirrored(H), _mirrored(W)
    num, den = torch.zeros_like(u), torch.zeros_like(u)
    for nb_u, nb_rho in ((u[up, :], rho[up, :]), (u[down, :], rho[down, :]), (u[:, left], rho[:, left]), (u[:, right], rho[:, right])):
        beta = 2.0 / (rho + nb_rho)
        num = num + beta * nb_u
        den = den + beta
    return torch.where(unknown_mask(H, W, mask), (num - h2 * rhs) / den, u)


def sweep(u, rho, rhs, dx, mask, n_sweeps=1, dtype=torch.float64):
    """-> the list of iterates u^0 .. u^n."""
    out = [_t(u, dtype)]
    rho, rhs = _t(rho, dtype), _t(rhs, dtype)
    for _ in range(int(n_sweeps)):
        out.append(sweep_once(out[-1], rho, rhs, dx, mask))
    return out


def autograd_grads(u, rho, rhs, dx, mask, n_sweeps, gbar):
    """torch.autograd through n sweeps of loss = sum(gbar * u^n) -> (u^n, {'u', 'rho', 'rhs'}), float64."""
    leaves = [_t(a).clone().requires_grad_(True) for a in (u, rho, rhs)]
    out = sweep(*leaves, dx, mask, n_sweeps)[-1]
    (out * _t(gbar)).sum().backward()
    return out.detach(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in zip(KEYS, leaves)}


def _faces(rho):
    """Per axis the faces between node a (lower index) and b = a + 1: (slices of a, slices of b, beta, m of a reading b, m of b reading a)."""
    out = []
    for ax in (0, 1):
        n = rho.shape[ax]
        lo, hi = [slice(None)] * 2, [slice(None)] * 2
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        shape = [1, 1]
        shape[ax] = n - 1
        ma, mb = torch.ones(n - 1, dtype=rho.dtype), torch.ones(n - 1, dtype=rho.dtype)
        ma[0], mb[-1] = 2.0, 2.0                           # node 0 / n-1 has no neighbour on its other side
        out.append((lo, hi, 2.0 / (rho[lo] + rho[hi]), ma.reshape(shape), mb.reshape(shape)))
    return out


def closed_form(u, rho, rhs, dx, mask, n_sweeps, gbar, dtype=torch.float64):
    """The hand-written backward of n sweeps, everything in `dtype` (the iterates too) -> {'u', 'rho', 'rhs'}."""
    with torch.no_grad():
        its = sweep(u, rho, rhs, dx, mask, n_sweeps, dtype)
        rho = _t(rho, dtype)
        H, W = rho.shape
        h2 = torch.tensor(float(dx), dtype=dtype) ** 2
        unk = unknown_mask(H, W, mask)
        faces = _faces(rho)
        diag = torch.zeros_like(rho)
        for lo, hi, beta, ma, mb in faces:
            diag[lo] += ma * beta
            diag[hi] += mb * beta
        g = _t(gbar, dtype).clone()
        drho, drhs = torch.zeros_like(rho), torch.zeros_like(rho)
        zero = torch.zeros_like(rho)
        for t in range(int(n_sweeps) - 1, -1, -1):
            old, new = its[t], its[t + 1]
            a = torch.where(unk, g / diag, zero)
            prev = torch.where(unk, zero, g)
            drhs -= h2 * a
            for lo, hi, beta, ma, mb in faces:
                prev[hi] += ma * beta * a[lo]
                prev[lo] += mb * beta * a[hi]
                share = -0.5 * beta * beta * (ma * a[lo] * (old[hi] - new[lo]) + mb * a[hi] * (old[lo] - new[hi]))
                drho[lo] += share
                drho[hi] += share
            g = prev
        return {'u': g, 'rho': drho, 'rhs': drhs}


def residual_loss(pred, rho, rhs, dx, mask, coef):
    """coef * sum over the unknowns of w (L pred - rhs)^2 (varcoef_pi_loss_partials), with the mirrored index lists of `sweep_once`; differentiable."""
    H, W = pred.shape
    h2 = torch.tensor(float(dx), dtype=pred.dtype) ** 2
    (up, down), (left, right) = _mirrored(H), _mirrored(W)
    s = torch.zeros_like(pred)
    for nb_u, nb_rho in ((pred[up, :], rho[up, :]), (pred[down, :], rho[down, :]), (pred[:, left], rho[:, left]), (pred[:, right], rho[:, right])):
        s = s + 2.0 / (rho + nb_rho) * (nb_u - pred)
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    w = torch.zeros((H, W), dtype=pred.dtype)
    w[i0:i1 + 1, j0:j1 + 1] = torch.as_tensor(B.weights(H, W, mask), dtype=pred.dtype)
    r = s / h2 - rhs
    return float(coef) * (w * r * r).sum()


def chain_autograd(u, rho, rhs, dx, mask, n_sweeps, coef):
    """d residual_loss(sweep^n(u, rho, rhs), rho, rhs) / d (u, rho, rhs) by torch.autograd through the whole chain, float64."""
    leaves = [_t(a).clone().requires_grad_(True) for a in (u, rho, rhs)]
    residual_loss(sweep(*leaves, dx, mask, n_sweeps)[-1], leaves[1], leaves[2], dx, mask, coef).backward()
    return {k: t.grad for k, t in zip(KEYS, leaves)}


def chain_closed_form(u, rho, rhs, dx, mask, n_sweeps, coef, dtype=torch.float64):
    """The same gradients the way the tape forms them, all in `dtype`: the residual's own gradients at the smoothed field, then `closed_form` with
    d loss / d pred as the smoother's incoming gradient; rho and rhs get both parts."""
    pred = sweep(u, rho, rhs, dx, mask, n_sweeps, dtype)[-1].detach()
    leaves = [t.clone().requires_grad_(True) for t in (pred, _t(rho, dtype), _t(rhs, dtype))]
    residual_loss(*leaves, dx, mask, coef).backward()
    g = closed_form(u, rho, rhs, dx, mask, n_sweeps, leaves[0].grad, dtype)
    return {'u': g['u'], 'rho': g['rho'] + leaves[1].grad, 'rhs': g['rhs'] + leaves[2].grad}


def rel_l2(a, b):
    a, b = _t(a).reshape(-1), _t(b).reshape(-1)
    nb = float(torch.linalg.norm(b))
    return float(torch.linalg.norm(a - b)) / nb if nb > 0 else float(torch.linalg.norm(a))


# ----------------------------------------------------------------------------- the inputs both suites use
def jump_density(rng, N, H, W, lo=1.0, hi=2.0, ratio=100.0):
    """Random in [lo, hi], times `ratio` below the diagonal of the field: a 100 : 1 jump that crosses every tile boundary."""
    rho = rng.uniform(lo, hi, (N, H, W))
    below = (np.arange(H)[:, None] * (W - 1)) > (np.arange(W)[None, :] * (H - 1))
    rho[:, below] *= ratio
    return rho


@functools.lru_cache(maxsize=None)
def case(H, W, N=3):
    """fp32-representable float64 host arrays (read-only): u, rho, rhs, gbar (N,H,W) and a different dx per sample (N,)."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    rng = np.random.default_rng(5000 * H + W)
    u, rhs, gbar = (f32(rng.standard_normal((N, H, W))) for _ in range(3))
    rho = f32(jump_density(rng, N, H, W))
    dx = f32(rng.uniform(5e-3, 5e-2, N))
    for a in (u, rho, rhs, gbar, dx):
        a.setflags(write=False)
    return u, rho, rhs, gbar, dx


@functools.lru_cache(maxsize=None)
def reference(H, W, mask, n_sweeps, N=3):
    """Per case, once: ({key: (N,H,W) float64 gradients by the closed form}, {key: rel-L2 of the float32 closed form against them - the floor})."""
    u, rho, rhs, gbar, dx = case(H, W, N)
    ref = [closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, gbar[n]) for n in range(N)]
    low = [closed_form(u[n], rho[n], rhs[n], dx[n], mask, n_sweeps, gbar[n], dtype=torch.float32) for n in range(N)]
    ref = {k: torch.stack([r[k] for r in ref]) for k in KEYS}
    return ref, {k: rel_l2(torch.stack([r[k] for r in low]), ref[k]) for k in KEYS}
