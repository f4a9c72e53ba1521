"""fp64 numpy / scipy twin of the variable-density Poisson solve (poisson_cnn_amd/csrc/varcoef.hip).

div((1/rho) grad u) = f on the vertex-centred H x W grid with spacing dx (dy = dx), Dirichlet data on the four edges, in the flux form
    beta_face = 2 / (rho_a + rho_b),   (A u)[i,j] = sum_neighbours beta_face (u[i,j] - u[neighbour]) / dx^2
on the (H-2) x (W-2) interior nodes (C order).  A u = b with b = -f + (Dirichlet neighbours' values times beta_face / dx^2).
Edge names as in oracle.dataset: left / right are rows 0 / H-1 (length W), bottom / top columns 0 / W-1 (length H)."""
import numpy as np
import scipy.fft
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def face_coefficients(rho):
    """rho (H,W) -> (beta_i (H-1,W): faces between rows i and i+1, beta_j (H,W-1): faces between columns j and j+1)."""
    rho = np.asarray(rho, dtype=np.float64)
    return 2.0 / (rho[:-1, :] + rho[1:, :]), 2.0 / (rho[:, :-1] + rho[:, 1:])


def assemble(rho, dx):
    """The sparse SPD matrix A ((H-2)(W-2) square, CSR)."""
    H, W = rho.shape
    nh, nw = H - 2, W - 2
    bi, bj = face_coefficients(rho)
    h2 = float(dx) ** 2
    lo_i, hi_i = bi[:-1, 1:-1] / h2, bi[1:, 1:-1] / h2        # faces of interior node (i, j) towards i-1 and i+1
    lo_j, hi_j = bj[1:-1, :-1] / h2, bj[1:-1, 1:] / h2        # ... towards j-1 and j+1
    idx = np.arange(nh * nw).reshape(nh, nw)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [(lo_i + hi_i + lo_j + hi_j).ravel()]
    rows += [idx[1:, :].ravel(), idx[:-1, :].ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel()]
    cols += [idx[:-1, :].ravel(), idx[1:, :].ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel()]
    vals += [-lo_i[1:, :].ravel(), -hi_i[:-1, :].ravel(), -lo_j[:, 1:].ravel(), -hi_j[:, :-1].ravel()]
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nh * nw, nh * nw))


def right_hand_side(rho, f, boundaries, dx):
    """b ((H-2)(W-2),) for one sample; boundaries: dict of 1-D arrays."""
    bi, bj = face_coefficients(rho)
    h2 = float(dx) ** 2
    b = -np.array(f, dtype=np.float64)[1:-1, 1:-1]
    b[0, :] += bi[0, 1:-1] / h2 * np.asarray(boundaries['left'], dtype=np.float64)[1:-1]
    b[-1, :] += bi[-1, 1:-1] / h2 * np.asarray(boundaries['right'], dtype=np.float64)[1:-1]
    b[:, 0] += bj[1:-1, 0] / h2 * np.asarray(boundaries['bottom'], dtype=np.float64)[1:-1]
    b[:, -1] += bj[1:-1, -1] / h2 * np.asarray(boundaries['top'], dtype=np.float64)[1:-1]
    return b.ravel()


def embed(u_int, boundaries, H, W):
    """Interior solution + edges, with the corner convention of oracle.dataset.multigrid_poisson_solve (left / right written last)."""
    out = np.zeros((H, W))
    out[1:-1, 1:-1] = np.asarray(u_int).reshape(H - 2, W - 2)
    out[:, -1] = boundaries['top']
    out[:, 0] = boundaries['bottom']
    out[0, :] = boundaries['left']
    out[-1, :] = boundaries['right']
    return out


def solve(rho, f, boundaries, dx):
    """Direct sparse solve of one sample -> (H,W)."""
    H, W = rho.shape
    u = spla.spsolve(assemble(rho, dx).tocsc(), right_hand_side(rho, f, boundaries, dx))
    return embed(u, boundaries, H, W)


def solve_batch(rho, f, boundaries, dx):
    """rho, f (N,H,W); boundaries dict of (N,len); dx (N,) -> (N,H,W)."""
    return np.stack([solve(rho[n], f[n], {k: v[n] for k, v in boundaries.items()}, dx[n]) for n in range(rho.shape[0])])


def dst_precondition(r, nh, nw):
    """z = M^-1 r, M the unit-spacing 5-point operator with zero Dirichlet data, by the orthonormal DST-I."""
    lam_h = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, nh + 1) / (nh + 1))
    lam_w = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, nw + 1) / (nw + 1))
    c = scipy.fft.dstn(r.reshape(nh, nw), type=1, norm='ortho') / (lam_h[:, None] + lam_w[None, :])
    return scipy.fft.dstn(c, type=1, norm='ortho').ravel()


def pcg(A, b, shape, tol=1e-10, max_iterations=500, x0=None):
    """The recurrence of the device loop: x += alpha p, r -= alpha q, stop at ||r|| <= tol ||b|| -> (x, iterations, ||r|| / ||b||)."""
    nh, nw = shape
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x
    bb = float(b @ b)
    if float(r @ r) <= tol * tol * bb:
        return x, 0, (np.sqrt(float(r @ r) / bb) if bb > 0 else 0.0)
    z = dst_precondition(r, nh, nw)
    p, rz = z.copy(), float(r @ z)
    it = 0
    while it < max_iterations:
        q = A @ p
        alpha = rz / float(p @ q)
        x += alpha * p
        r -= alpha * q
        it += 1
        if float(r @ r) <= tol * tol * bb:
            break
        z = dst_precondition(r, nh, nw)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it, np.sqrt(float(r @ r) / bb)


def smooth_density(rng, H, W, lo, hi, modes=3):
    """A smooth positive field with min = lo and max = hi exactly: a few random cosine modes, rescaled."""
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing='ij')
    g = sum(rng.uniform(-1, 1) * np.cos(np.pi * (a * y + rng.uniform())) * np.cos(np.pi * (b * x + rng.uniform())) for a in range(1, modes + 1) for b in range(1, modes + 1))
    g = (g - g.min()) / (g.max() - g.min())
    return lo + (hi - lo) * g
