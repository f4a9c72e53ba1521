"""torch float64 CPU twin of the differentiable variable-density solve (poisson_cnn_amd/csrc/varcoef_grad.hip, autograd.variable_density_solve /
variable_density_residual), in the notation of tests/varcoef_bc_twin.py.

Two independent routes to every gradient:
  * `assemble` builds the dense A(rho) and b(rho, f, edges) of varcoef_bc_twin.assemble from differentiable torch ops (the same node-by-node index
    lists, the values as tensors), `solve` is torch.linalg.solve plus the embedding, and torch.autograd differentiates through all of it
    (`solve_grads`, `loss_grads`);
  * `closed_form` / `loss_closed_form` are the hand-written gather formulas the kernels implement, on whole-array slices: with lam the adjoint
    (A^T lam = du on the unknowns, 0 elsewhere), beta = 2 / (rho_a + rho_b), m = 2 where c is a Neumann edge node and k its inward neighbour,
        d rho_p  = sum over faces (c,k) touching p of 1/2 beta^2 m lam_c (u_c - u_k) / h^2  -  lam_p sum_e 2 g_e / (rho_p^2 h)
        d f      = -lam
        d value of Dirichlet node d = du_d + sum over neighbours c of lam_c m beta / h^2 (0 for an array entry the writer overwrites at a corner)
        d g_e at edge node c        = lam_c 2 / (rho_c h)
    and for the loss sum w r^2 * coef, r = L u - f:  lam = 2 coef w r  (no solve).
`closed_form` takes any float dtype: run in float32 it is the floor of an fp32 evaluation of the same formulas."""
import functools

import numpy as np
import torch

from tests import varcoef_bc_twin as B

EDGES = B.EDGES


def _t(a, dtype=torch.float64):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=dtype)


def dirichlet_field(edges, H, W, mask, dtype=torch.float64):
    """varcoef_bc_twin.dirichlet_field with tensors: the in-place writes keep the writer's order, so an overwritten entry gets no gradient."""
    nl, nr, nb, nt = B.flags(mask)
    g = torch.zeros((H, W), dtype=dtype)
    if not nt:
        g[:, -1] = edges['top']
    if not nb:
        g[:, 0] = edges['bottom']
    if not nl:
        g[0, :] = edges['left']
    if not nr:
        g[-1, :] = edges['right']
    return g


@functools.lru_cache(maxsize=None)
def _stencil(H, W, mask):
    """The entries of varcoef_bc_twin.assemble as index lists: per (unknown c, existing neighbour k) its row, both nodes, m, and k's column or -1."""
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    mw = j1 - j0 + 1
    row, ci, cj, ki, kj, m, col = [], [], [], [], [], [], []
    for i in range(i0, i1 + 1):
        for j in range(j0, j1 + 1):
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                a, k = i + di, j + dj
                if a < 0 or a >= H or k < 0 or k >= W:
                    continue
                row.append((i - i0) * mw + (j - j0)); ci.append(i); cj.append(j); ki.append(a); kj.append(k)
                m.append(1.0 if (0 <= i - di < H and 0 <= j - dj < W) else 2.0)
                col.append((a - i0) * mw + (k - j0) if (i0 <= a <= i1 and j0 <= k <= j1) else -1)
    return tuple(torch.tensor(v) for v in (row, ci, cj, ki, kj)) + (torch.tensor(m, dtype=torch.float64), torch.tensor(col))


def assemble(rho, dx, mask, edges, f):
    """-> (A (n,n) dense, b (n,)), differentiable in rho, f and the edge arrays."""
    rho, f = _t(rho), _t(f)
    e = {k: _t(edges[k]) for k in EDGES}
    H, W = rho.shape
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    n = (i1 - i0 + 1) * (j1 - j0 + 1)
    h = float(dx)
    row, ci, cj, ki, kj, m, col = _stencil(H, W, mask)
    beta = m * 2.0 / (rho[ci, cj] + rho[ki, kj]) / h ** 2
    dval = dirichlet_field(e, H, W, mask)
    unk = col >= 0
    A = torch.zeros((n, n), dtype=torch.float64)
    A = A.index_put((row, row), beta, accumulate=True)
    A = A.index_put((row[unk], col[unk]), -beta[unk], accumulate=True)
    b = -f[i0:i1 + 1, j0:j1 + 1].reshape(-1)
    b = b.index_put((row[~unk],), beta[~unk] * dval[ki[~unk], kj[~unk]], accumulate=True)
    bn = torch.zeros((H, W), dtype=torch.float64)
    nl, nr, nb, nt = B.flags(mask)
    gn = 2.0 / (rho * h)
    if nl:
        bn[0, :] += gn[0, :] * e['left']
    if nr:
        bn[-1, :] += gn[-1, :] * e['right']
    if nb:
        bn[:, 0] += gn[:, 0] * e['bottom']
    if nt:
        bn[:, -1] += gn[:, -1] * e['top']
    return A, b + bn[i0:i1 + 1, j0:j1 + 1].reshape(-1)


def embed(u, edges, H, W, mask):
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    out = dirichlet_field({k: _t(edges[k]) for k in EDGES}, H, W, mask)
    out[i0:i1 + 1, j0:j1 + 1] = u.reshape(i1 - i0 + 1, j1 - j0 + 1)
    return out


def solve(rho, f, edges, dx, mask):
    """One sample -> the (H,W) field; mask 15 is singular and not handled."""
    A, b = assemble(rho, dx, mask, edges, f)
    H, W = np.shape(rho)
    return embed(torch.linalg.solve(A, b), edges, H, W, mask)


def _leaves(rho, f, edges):
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    return leaf(rho), leaf(f), {k: leaf(edges[k]) for k in EDGES}


def solve_grads(rho, f, edges, dx, mask, ubar):
    """autograd through the dense solve of loss = sum(ubar * u) -> (u, {'rho', 'rhs', 'left', 'right', 'bottom', 'top'})."""
    r, ff, e = _leaves(rho, f, edges)
    u = solve(r, ff, e, dx, mask)
    (u * _t(ubar)).sum().backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return u.detach(), dict({'rho': z(r), 'rhs': z(ff)}, **{k: z(e[k]) for k in EDGES})


def adjoint(rho, dx, mask, ubar):
    """lam (H,W): A^T lam = ubar on the unknowns, 0 on Dirichlet nodes."""
    H, W = np.shape(rho)
    zero = {k: torch.zeros(W if k in ('left', 'right') else H, dtype=torch.float64) for k in EDGES}
    A, _ = assemble(rho, dx, mask, zero, torch.zeros((H, W), dtype=torch.float64))
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    lam = torch.zeros((H, W), dtype=torch.float64)
    lam[i0:i1 + 1, j0:j1 + 1] = torch.linalg.solve(A.T, _t(ubar)[i0:i1 + 1, j0:j1 + 1].reshape(-1)).reshape(i1 - i0 + 1, j1 - j0 + 1)
    return lam


def _faces(lam, u, rho, h):
    """Per axis the faces between node a (lower index) and node b = a + 1: (beta, u_a - u_b, m_ab lam_a, m_ba lam_b), m = 2 where the node has no
    neighbour on its other side (only an unknown on a Neumann edge has lam != 0 there)."""
    out = []
    for ax in (0, 1):
        n = lam.shape[ax]
        lo, hi = [slice(None)] * 2, [slice(None)] * 2
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        shape = [1, 1]
        shape[ax] = n - 1
        ma, mb = torch.ones(n - 1, dtype=lam.dtype), torch.ones(n - 1, dtype=lam.dtype)
        ma[0], mb[-1] = 2.0, 2.0
        beta = 2.0 / (rho[lo] + rho[hi])
        out.append((lo, hi, beta, u[lo] - u[hi], ma.reshape(shape) * lam[lo], mb.reshape(shape) * lam[hi]))
    return out


def closed_form(lam, u, rho, dx, mask, edges=None, du=None, dtype=torch.float64):
    """The gather formulas on one sample.  lam (H,W) zero off the unknowns, u the full field, edges: the Neumann data (None: zero; entries of Dirichlet
    edges are not read), du: the direct term of the edge gradient (None: zero).  -> {'rho', 'rhs', 'left', 'right', 'bottom', 'top'} in `dtype`."""
    lam, u, rho = _t(lam, dtype), _t(u, dtype), _t(rho, dtype)
    H, W = rho.shape
    h = torch.tensor(float(dx), dtype=dtype)
    inv_h2 = 1.0 / (h * h)
    nl, nr, nb, nt = B.flags(mask)
    drho = torch.zeros_like(rho)
    G = torch.zeros_like(rho) if du is None else _t(du, dtype).clone()
    for lo, hi, beta, d, la, lb in _faces(lam, u, rho, h):
        t = 0.5 * beta * beta * d * (la - lb) * inv_h2
        drho[lo] += t
        drho[hi] += t
        G[hi] += la * beta * inv_h2
        G[lo] += lb * beta * inv_h2
    if edges is not None:
        e = {k: _t(edges[k], dtype) for k in EDGES}
        s = 2.0 / (rho * rho * h)
        if nl:
            drho[0, :] -= lam[0, :] * s[0, :] * e['left']
        if nr:
            drho[-1, :] -= lam[-1, :] * s[-1, :] * e['right']
        if nb:
            drho[:, 0] -= lam[:, 0] * s[:, 0] * e['bottom']
        if nt:
            drho[:, -1] -= lam[:, -1] * s[:, -1] * e['top']
    gn = lam * 2.0 / (rho * h)
    out = {'rho': drho, 'rhs': -lam,
           'left': (gn if nl else G)[0, :].clone(), 'right': (gn if nr else G)[-1, :].clone(),
           'bottom': (gn if nb else G)[:, 0].clone(), 'top': (gn if nt else G)[:, -1].clone()}
    for k, dirichlet in (('bottom', not nb), ('top', not nt)):        # rows 0 / H-1 are written last: a Dirichlet row owns its corners
        if dirichlet and not nl:
            out[k][0] = 0.0
        if dirichlet and not nr:
            out[k][-1] = 0.0
    return out


def unknown_mask(H, W, mask):
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    m = torch.zeros((H, W), dtype=torch.bool)
    m[i0:i1 + 1, j0:j1 + 1] = True
    return m


def weight_field(H, W, mask, dtype=torch.float64):
    """w on the unknowns, 0 elsewhere, (H,W)."""
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    w = torch.zeros((H, W), dtype=dtype)
    w[i0:i1 + 1, j0:j1 + 1] = torch.as_tensor(B.weights(H, W, mask), dtype=dtype)
    return w


def loss_closed_form(pred, rho, rhs, dx, mask, coef, dtype=torch.float64):
    """d(coef sum w r^2) / d(rhs, rho), r = L pred - rhs on the unknowns with du/dn = 0 on Neumann edges -> (loss, {'rhs', 'rho'})."""
    u, rho, f = _t(pred, dtype), _t(rho, dtype), _t(rhs, dtype)
    H, W = rho.shape
    h = torch.tensor(float(dx), dtype=dtype)
    inv_h2 = 1.0 / (h * h)
    ones = torch.ones_like(u)
    S = torch.zeros_like(u)
    for lo, hi, beta, d, ma, mb in _faces(ones, u, rho, h):
        S[lo] -= ma * beta * d
        S[hi] += mb * beta * d
    w = weight_field(H, W, mask, dtype)
    r = torch.where(w > 0, S * inv_h2 - f, torch.zeros_like(u))
    lam = 2.0 * float(coef) * w * r
    g = closed_form(lam, u, rho, dx, mask, None, None, dtype)
    return float(coef) * (w * r * r).sum(), {'rhs': g['rhs'], 'rho': g['rho']}


def loss_grads(pred, rho, rhs, dx, mask, coef):
    """autograd of coef * sum w (b - A x)^2 through `assemble`, the field's own Dirichlet values and du/dn = 0 as edge data -> (loss, {'rhs', 'rho'})."""
    pred = _t(pred)
    H, W = pred.shape
    nl, nr, nb, nt = B.flags(mask)
    own = {'left': pred[0, :], 'right': pred[-1, :], 'bottom': pred[:, 0], 'top': pred[:, -1]}
    edges = {k: (torch.zeros_like(own[k]) if n else own[k]) for k, n in zip(EDGES, (nl, nr, nb, nt))}
    r, f, _ = _leaves(rho, rhs, edges)
    A, b = assemble(r, dx, mask, edges, f)
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    res = b - A @ pred[i0:i1 + 1, j0:j1 + 1].reshape(-1)
    loss = float(coef) * (torch.as_tensor(B.weights(H, W, mask)).reshape(-1) * res * res).sum()
    loss.backward()
    return loss.detach(), {'rhs': f.grad, 'rho': r.grad}


def rel_l2(a, b):
    a, b = _t(a).reshape(-1), _t(b).reshape(-1)
    nb = float(torch.linalg.norm(b))
    return float(torch.linalg.norm(a - b)) / nb if nb > 0 else float(torch.linalg.norm(a))


# ----------------------------------------------------------------------------- the density-identification sanity problem of the GPU suite
GD_SHAPE, GD_DX, GD_STEPS = (17, 65), 1.0 / 64.0, 10
GD_STEP = 40.0          # chosen on this twin: the objective falls at every one of the ten steps for 46.6 (0.25 / max|gradient| at the start) and rises from
#                         the third step on for 186; tests/test_varcoef_grad_reference.py checks 40


def gd_problem():
    """(rho_true in [1, 3], rhs, zero Dirichlet edges, u_true) float64 tensors, fp32-representable: recover rho from u_true starting at rho = 2."""
    H, W = GD_SHAPE
    y = torch.arange(H, dtype=torch.float64)[:, None] / (H - 1)
    x = torch.arange(W, dtype=torch.float64)[None, :] / (W - 1)
    f32 = lambda t: t.to(torch.float32).to(torch.float64)
    rho_true = f32(2.0 + torch.sin(2.0 * np.pi * x) * torch.cos(np.pi * y))
    rhs = f32(-10.0 * (1.0 + x) * torch.sin(np.pi * y) * torch.ones_like(x))
    edges = {k: torch.zeros(W if k in ('left', 'right') else H, dtype=torch.float64) for k in EDGES}
    u_true = f32(solve(rho_true, rhs, edges, GD_DX, 0).detach())
    return rho_true, rhs, edges, u_true


def gd_objective_and_grad(rho, rhs, edges, u_true):
    r = _t(rho).clone().requires_grad_(True)
    obj = (solve(r, rhs, edges, GD_DX, 0) - u_true).square().sum()
    obj.backward()
    return float(obj.detach()), r.grad


def gd_run(step, steps=GD_STEPS):
    """Plain gradient descent from rho = 2 -> the objective before each step and after the last (steps + 1 values)."""
    rho_true, rhs, edges, u_true = gd_problem()
    rho = torch.full(GD_SHAPE, 2.0, dtype=torch.float64)
    hist = []
    for _ in range(steps):
        obj, g = gd_objective_and_grad(rho, rhs, edges, u_true)
        hist.append(obj)
        rho = rho - step * g
    hist.append(gd_objective_and_grad(rho, rhs, edges, u_true)[0])
    return hist
