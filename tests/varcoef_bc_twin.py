"""fp64 numpy / scipy twin of the variable-density Poisson solve with per-edge Dirichlet / Neumann boundaries (the *_bc_* entry points of
poisson_cnn_amd/csrc/varcoef.hip); tests/varcoef_twin.py is its all-Dirichlet case.

div((1/rho) grad u) = f on the vertex-centred H x W grid, spacing dx (dy = dx).  mask bit 0/1/2/3 = left / right / bottom / top is Neumann (left /
right are rows 0 / H-1, bottom / top columns 0 / W-1): such an edge's array holds g = du/dn along the outward normal and its nodes are unknowns; a
Dirichlet edge wins a corner.  Unknowns: rows i0..i1 x columns j0..j1 (C order).  With beta_face = 2 / (rho_a + rho_b):
    (A u)_c = sum over the four directions of beta_k (u_c - u_k) / dx^2; beyond a Neumann edge the inward face of that direction counts twice
    b_c     = -f_c + beta_k / dx^2 * (value of each Dirichlet neighbour) + 2 g / (rho_c dx) for each Neumann edge the node lies on
    w       = w_i w_j, 1/2 on a Neumann edge's row / column: W A is symmetric."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EDGES = ('left', 'right', 'bottom', 'top')


def flags(mask):
    return tuple(bool(mask >> k & 1) for k in range(4))


def types(mask):
    return {e: ('neumann' if f else 'dirichlet') for e, f in zip(EDGES, flags(mask))}


def unknowns(H, W, mask):
    """(i0, i1, j0, j1), inclusive."""
    nl, nr, nb, nt = flags(mask)
    return (0 if nl else 1), (H - 1 if nr else H - 2), (0 if nb else 1), (W - 1 if nt else W - 2)


def weights(H, W, mask):
    """w (mh, mw)."""
    i0, i1, j0, j1 = unknowns(H, W, mask)
    nl, nr, nb, nt = flags(mask)
    wi, wj = np.ones(i1 - i0 + 1), np.ones(j1 - j0 + 1)
    if nl:
        wi[0] = 0.5
    if nr:
        wi[-1] = 0.5
    if nb:
        wj[0] = 0.5
    if nt:
        wj[-1] = 0.5
    return wi[:, None] * wj[None, :]


def dirichlet_field(boundaries, H, W, mask):
    """The values the Dirichlet nodes have (0 elsewhere): what the solvers' writer puts there - columns first, then rows 0 / H-1, which win a
    corner between two Dirichlet edges; a Neumann edge's array holds no values and a Dirichlet edge wins the corner it shares with one."""
    nl, nr, nb, nt = flags(mask)
    g = np.zeros((H, W))
    if not nt:
        g[:, -1] = boundaries['top']
    if not nb:
        g[:, 0] = boundaries['bottom']
    if not nl:
        g[0, :] = boundaries['left']
    if not nr:
        g[-1, :] = boundaries['right']
    return g


def assemble(rho, dx, mask, boundaries=None, f=None):
    """-> (A (CSR, mh mw square), b or None): node by node, straight from the definition."""
    rho = np.asarray(rho, dtype=np.float64)
    H, W = rho.shape
    i0, i1, j0, j1 = unknowns(H, W, mask)
    mh, mw = i1 - i0 + 1, j1 - j0 + 1
    h = float(dx)
    h2 = float(dx) ** 2                                              # (the spelling of tests/varcoef_twin.py: mask 0 gives its numbers exactly)
    nl, nr, nb, nt = flags(mask)
    want_b = boundaries is not None
    if want_b:
        e = {k: np.asarray(boundaries[k], dtype=np.float64) for k in EDGES}
        dval = dirichlet_field(e, H, W, mask)
        b = -np.asarray(f, dtype=np.float64)[i0:i1 + 1, j0:j1 + 1].copy()
    rows, cols, vals = [], [], []
    is_unknown = lambda i, j: i0 <= i <= i1 and j0 <= j <= j1
    for i in range(i0, i1 + 1):
        for j in range(j0, j1 + 1):
            c = (i - i0) * mw + (j - j0)
            diag = 0.0
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                a, k = i + di, j + dj
                if a < 0 or a >= H or k < 0 or k >= W:
                    continue                                         # no outward neighbour: its share is the doubled inward face below
                beta = 2.0 / (rho[i, j] + rho[a, k]) / h2
                opposite_missing = not (0 <= i - di < H and 0 <= j - dj < W)
                if opposite_missing:
                    beta *= 2.0                                      # this is the inward face of a Neumann edge node
                diag += beta
                if is_unknown(a, k):
                    rows.append(c); cols.append((a - i0) * mw + (k - j0)); vals.append(-beta)
                elif want_b:
                    b[i - i0, j - j0] += beta * dval[a, k]
            rows.append(c); cols.append(c); vals.append(diag)
            if want_b:
                gn = 2.0 / (rho[i, j] * h)
                if i == 0:
                    b[i - i0, j - j0] += gn * e['left'][j]
                if i == H - 1:
                    b[i - i0, j - j0] += gn * e['right'][j]
                if j == 0:
                    b[i - i0, j - j0] += gn * e['bottom'][i]
                if j == W - 1:
                    b[i - i0, j - j0] += gn * e['top'][i]
    A = sp.csr_matrix((vals, (rows, cols)), shape=(mh * mw, mh * mw))
    return A, (b.ravel() if want_b else None)


def embed(u, boundaries, H, W, mask):
    i0, i1, j0, j1 = unknowns(H, W, mask)
    out = dirichlet_field({k: np.asarray(boundaries[k], dtype=np.float64) for k in EDGES}, H, W, mask)
    out[i0:i1 + 1, j0:j1 + 1] = np.asarray(u).reshape(i1 - i0 + 1, j1 - j0 + 1)
    return out


def project(b, w):
    """mask 15: (b - sum w b / sum w, compatibility defect |sum w b| / sqrt(sum w * sum w b^2), the constant taken off)."""
    w = w.ravel()
    m = float(w @ b) / float(w.sum())
    defect = abs(float(w @ b)) / np.sqrt(float(w.sum()) * float(w @ (b * b)))
    return b - m, defect, m


def solve(rho, f, boundaries, dx, mask):
    """Direct sparse solve of one sample -> (H,W).  mask 15: the projected system, the solution with zero w-mean (a Lagrange multiplier row)."""
    H, W = rho.shape
    A, b = assemble(rho, dx, mask, boundaries, f)
    if mask != 15:
        return embed(spla.spsolve(A.tocsc(), b), boundaries, H, W, mask)
    w = weights(H, W, mask).ravel()
    bp = project(b, weights(H, W, mask))[0]
    n = A.shape[0]
    K = sp.bmat([[sp.diags(w) @ A, sp.csr_matrix(w[:, None])], [sp.csr_matrix(w[None, :]), None]], format='csc')
    u = spla.spsolve(K, np.concatenate([w * bp, [0.0]]))[:n]
    return embed(u, boundaries, H, W, mask)


def solve_batch(rho, f, boundaries, dx, mask):
    return np.stack([solve(rho[n], f[n], {k: v[n] for k, v in boundaries.items()}, dx[n], mask) for n in range(rho.shape[0])])


def axis_basis(n, neumann_lo, neumann_hi):
    """(Vinv, V, lam) of the 1-D constant-coefficient operator on an n-point axis' unknowns, V^T W V = I (dataset/_kernels.py axis_decomposition)."""
    m = n - 2 + int(neumann_lo) + int(neumann_hi)
    M = 2.0 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)
    w = np.ones(m)
    if neumann_lo:
        M[0, 1], w[0] = -2.0, 0.5
    if neumann_hi:
        M[m - 1, m - 2], w[m - 1] = -2.0, 0.5
    lam, V = scipy.linalg.eigh(np.diag(w) @ M, np.diag(w))
    if neumann_lo and neumann_hi:
        lam[0] = 0.0
    return V.T * w[None, :], V, lam, M


def constant_operator(H, W, mask):
    """The unit-spacing constant-coefficient operator M of pcnn_fd_poisson_mixed on the unknowns (dense Kronecker sum)."""
    nl, nr, nb, nt = flags(mask)
    Mh, Mw = axis_basis(H, nl, nr)[3], axis_basis(W, nb, nt)[3]
    return np.kron(Mh, np.eye(Mw.shape[0])) + np.kron(np.eye(Mh.shape[0]), Mw)


def preconditioner(H, W, mask):
    """r (mh mw,) -> z = V_h ((Vinv_h r Vinv_w^T) ./ (lam_h + lam_w)) V_w^T, the lam = 0 mode dropped."""
    nl, nr, nb, nt = flags(mask)
    Vih, Vh, lh, _ = axis_basis(H, nl, nr)
    Viw, Vw, lw, _ = axis_basis(W, nb, nt)
    lam = lh[:, None] + lw[None, :]
    keep = np.abs(lam) > 1e-13
    inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)

    def apply(r):
        c = Vih @ r.reshape(len(lh), len(lw)) @ Viw.T
        return (Vh @ (c * inv) @ Vw.T).ravel()
    return apply


def pcg(A, b, H, W, mask, tol=1e-10, max_iterations=500, x0=None):
    """The device loop: PCG in the W inner product; mask 15 projects b first and removes the w-mean of x at the end.
    -> (x, iterations, sqrt(sum w r^2 / sum w b^2))."""
    w = weights(H, W, mask).ravel()
    if mask == 15:
        b = project(b, weights(H, W, mask))[0]
    dot = lambda a, c: float(w @ (a * c))
    minv = preconditioner(H, W, mask)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x
    bb = dot(b, b)
    it = 0
    if dot(r, r) > tol * tol * bb:
        z = minv(r)
        p, rz = z.copy(), dot(r, z)
        while it < max_iterations:
            q = A @ p
            alpha = rz / dot(p, q)
            x += alpha * p
            r -= alpha * q
            it += 1
            if dot(r, r) <= tol * tol * bb:
                break
            z = minv(r)
            rz_new = dot(r, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
    if mask == 15:
        x = x - float(w @ x) / float(w.sum())
    return x, it, (np.sqrt(dot(r, r) / bb) if bb > 0 else 0.0)
