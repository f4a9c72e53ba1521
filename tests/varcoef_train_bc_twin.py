"""fp64 numpy / scipy twin of the training-side operators of the variable-density problem with per-edge Dirichlet / Neumann boundaries (the *_bc_*
entry points of poisson_cnn_amd/csrc/varcoef_train.hip), built on tests/varcoef_bc_twin.py; tests/varcoef_train_twin.py is its
all-Dirichlet case.

One sample: fields (H,W) float64, spacing dx, mask bit 0/1/2/3 = left / right / bottom / top is Neumann with du/dn = 0.  The unknowns are
varcoef_bc_twin.unknowns(H, W, mask); every other node is a Dirichlet node and keeps whatever the field holds there.
    residual  r = b - A x with varcoef_bc_twin.assemble(rho, dx, mask, the field's own Dirichlet edge values, f), x the field's unknowns
    loss      sum w r^2, w = varcoef_bc_twin.weights
    gradient  2 L^T (w r) on all nodes, L the (unknowns x H W) matrix assembled here node by node from the definition
              (L u)_c = sum_k m_k beta_k (u_k - u_c) / dx^2, m = 2 on the inward face of a Neumann edge node in that edge's direction
    sweep     J u + c: row c of J is the off-diagonal part of L over its diagonal on an unknown, the identity on a Dirichlet node
    adjoint   the literal transpose J^T."""
import numpy as np
import scipy.sparse as sp

from tests import varcoef_bc_twin as B


def own_edges(field, mask):
    """The solver's boundary arrays of a field: its own values on a Dirichlet edge, du/dn = 0 on a Neumann one."""
    f = np.asarray(field, dtype=np.float64)
    own = {'left': f[0, :], 'right': f[-1, :], 'bottom': f[:, 0], 'top': f[:, -1]}
    return {e: (np.zeros_like(own[e]) if neumann else own[e].copy()) for e, neumann in zip(B.EDGES, B.flags(mask))}


def unknown_slices(H, W, mask):
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    return slice(i0, i1 + 1), slice(j0, j1 + 1)


def operator_matrix(rho, dx, mask):
    """-> (L (CSR, unknowns x H W), diag (unknowns,): sum_k m_k beta_k / dx^2 of each unknown), from the definition, node by node."""
    rho = np.asarray(rho, dtype=np.float64)
    H, W = rho.shape
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    mw = j1 - j0 + 1
    h2 = float(dx) ** 2
    rows, cols, vals, diag = [], [], [], []
    for i in range(i0, i1 + 1):
        for j in range(j0, j1 + 1):
            c = (i - i0) * mw + (j - j0)
            d = 0.0
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                a, k = i + di, j + dj
                if not (0 <= a < H and 0 <= k < W):
                    continue                                          # a Neumann edge node: no outward neighbour
                m = 1.0 if (0 <= i - di < H and 0 <= j - dj < W) else 2.0      # ... and its inward face counts twice
                beta = m * 2.0 / (rho[i, j] + rho[a, k]) / h2
                rows.append(c); cols.append(a * W + k); vals.append(beta)
                d += beta
            rows.append(c); cols.append(i * W + j); vals.append(-d)
            diag.append(d)
    n = (i1 - i0 + 1) * mw
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, H * W)), np.array(diag)


def residual(pred, rho, rhs, dx, mask):
    """b - A x on the unknowns, (mh, mw): the solver's system with the field's own Dirichlet edge values."""
    pred = np.asarray(pred, dtype=np.float64)
    H, W = pred.shape
    A, b = B.assemble(rho, dx, mask, own_edges(pred, mask), rhs)
    si, sj = unknown_slices(H, W, mask)
    return (b - A @ pred[si, sj].ravel()).reshape(pred[si, sj].shape)


def loss(pred, rho, rhs, dx, mask):
    r = residual(pred, rho, rhs, dx, mask)
    return float((B.weights(pred.shape[0], pred.shape[1], mask) * r * r).sum())


def loss_grad(pred, rho, rhs, dx, mask):
    """d loss / d pred on all nodes, (H,W): 2 L^T (w r) with the explicit sparse transpose."""
    H, W = np.shape(pred)
    L, _ = operator_matrix(rho, dx, mask)
    wr = (B.weights(H, W, mask) * residual(pred, rho, rhs, dx, mask)).ravel()
    return (2.0 * (L.T @ wr)).reshape(H, W)


def sweep_matrix(rho, dx, mask):
    """-> (J (CSR, H W square), scale (H W,)): one sweep is J u - scale * rhs; scale = dx^2 / (sum_k m_k beta_k) on unknowns, 0 on Dirichlet nodes."""
    rho = np.asarray(rho, dtype=np.float64)
    H, W = rho.shape
    L, diag = operator_matrix(rho, dx, mask)
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    node = (np.arange(i0, i1 + 1)[:, None] * W + np.arange(j0, j1 + 1)[None, :]).ravel()           # the node of each unknown
    off = (L + sp.csr_matrix((diag, (np.arange(len(node)), node)), shape=L.shape)).tocsr()        # the diagonal removed
    off.eliminate_zeros()
    is_unknown = np.zeros(H * W, dtype=bool)
    is_unknown[node] = True
    P = sp.csr_matrix((np.ones(len(node)), (node, np.arange(len(node)))), shape=(H * W, len(node)))  # unknown -> node
    J = P @ sp.diags(1.0 / diag) @ off + sp.diags((~is_unknown).astype(np.float64))
    scale = np.zeros(H * W)
    scale[node] = 1.0 / diag                                          # (diag carries 1 / dx^2: dx^2 rhs / (sum m beta) = rhs / diag)
    return J.tocsr(), scale


def sweep(u, rho, rhs, dx, mask, n_sweeps=1):
    u = np.asarray(u, dtype=np.float64)
    J, scale = sweep_matrix(rho, dx, mask)
    c = scale * np.asarray(rhs, dtype=np.float64).ravel()
    x = u.ravel().copy()
    for _ in range(int(n_sweeps)):
        x = J @ x - c
    return x.reshape(u.shape)


def sweep_adjoint(g, rho, dx, mask, n_sweeps=1):
    g = np.asarray(g, dtype=np.float64)
    Jt = sweep_matrix(rho, dx, mask)[0].T.tocsr()
    x = g.ravel().copy()
    for _ in range(int(n_sweeps)):
        x = Jt @ x
    return x.reshape(g.shape)


# ----------------------------------------------------------------------------- batches (N,H,W), dx (N,)
def _each(fn, *fields, dx, mask, **kw):
    return np.stack([fn(*(np.asarray(f)[n] for f in fields), float(np.asarray(dx).reshape(-1)[n]), mask, **kw) for n in range(len(fields[0]))])


def loss_batch(pred, rho, rhs, dx, mask):
    return _each(loss, pred, rho, rhs, dx=dx, mask=mask)


def loss_grad_batch(pred, rho, rhs, dx, mask, coef):
    return np.asarray(coef, dtype=np.float64).reshape(-1, 1, 1) * _each(loss_grad, pred, rho, rhs, dx=dx, mask=mask)


def sweep_batch(u, rho, rhs, dx, mask, n_sweeps=1):
    return _each(sweep, u, rho, rhs, dx=dx, mask=mask, n_sweeps=n_sweeps)


def sweep_adjoint_batch(g, rho, dx, mask, n_sweeps=1):
    return _each(sweep_adjoint, g, rho, dx=dx, mask=mask, n_sweeps=n_sweeps)


def weight_sum(H, W, mask):
    return float(B.weights(H, W, mask).sum())


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
