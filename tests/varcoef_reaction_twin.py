"""fp64 numpy / scipy twin of the variable-density solve with a reaction term (the *_reaction entry points of poisson_cnn_amd/csrc/varcoef.hip,
DESIGN.md section 26), built on tests/varcoef_bc_twin.py, whose system it extends and never copies.

div((1/rho) grad u) - c u = f, c >= 0 on every node and read on the unknowns: (A + C) u = b with the A, b and w of varcoef_bc_twin and C = diag(c).
W (A + C) is symmetric, and positive definite once an edge is Dirichlet or c > 0 somewhere - mask 15 included: nothing is projected, no mean removed.
Preconditioner: the constant-coefficient solve of bbar M + cbar I, M the unit-coefficient operator of the same edge types WITH its 1 / dx^2, bbar
and cbar the w-weighted means of 1 / rho and of c over the unknowns."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import varcoef_bc_twin as B

EDGES = B.EDGES


def on_unknowns(field, mask):
    """(H,W) -> (mh, mw)."""
    H, W = field.shape
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    return np.asarray(field, dtype=np.float64)[i0:i1 + 1, j0:j1 + 1]


def assemble(rho, c, dx, mask, boundaries=None, f=None):
    """-> (A + C (CSR), b or None): varcoef_bc_twin's A and b, c added on the diagonal."""
    A, b = B.assemble(rho, dx, mask, boundaries, f)
    return (A + sp.diags(on_unknowns(c, mask).ravel())).tocsr(), b


def means(rho, c, mask):
    """(cbar, bbar): sum w c / sum w and sum w (1 / rho) / sum w over the unknowns."""
    w = B.weights(*rho.shape, mask)
    return float((w * on_unknowns(c, mask)).sum() / w.sum()), float((w / on_unknowns(rho, mask)).sum() / w.sum())


def solve(rho, c, f, boundaries, dx, mask):
    """Direct sparse solve of one sample -> (H,W); no projection and no mean removal for any mask."""
    H, W = rho.shape
    A, b = assemble(rho, c, dx, mask, boundaries, f)
    return B.embed(spla.spsolve(A.tocsc(), b), boundaries, H, W, mask)


def solve_batch(rho, c, f, boundaries, dx, mask):
    return np.stack([solve(rho[n], c[n], f[n], {k: v[n] for k, v in boundaries.items()}, dx[n], mask) for n in range(rho.shape[0])])


def preconditioner(H, W, mask, dx, cbar, bbar):
    """r (mh mw,) -> z = V_h ((Vinv_h r Vinv_w^T) ./ (bbar (lam_h + lam_w) / dx^2 + cbar)) V_w^T; the lam = 0 mode is dropped only when cbar = 0."""
    nl, nr, nb, nt = B.flags(mask)
    Vih, Vh, lh, _ = B.axis_basis(H, nl, nr)
    Viw, Vw, lw, _ = B.axis_basis(W, nb, nt)
    lam = lh[:, None] + lw[None, :]
    keep = (np.abs(lam) > 1e-13) | (cbar > 0.0)
    den = bbar / (float(dx) * float(dx)) * lam + cbar
    inv = np.where(keep, 1.0 / np.where(keep, den, 1.0), 0.0)

    def apply(r):
        t = Vih @ r.reshape(len(lh), len(lw)) @ Viw.T
        return (Vh @ (t * inv) @ Vw.T).ravel()
    return apply


def preconditioner_matrix(H, W, mask, dx, cbar, bbar):
    """bbar M / dx^2 + cbar I, dense, M = varcoef_bc_twin.constant_operator: what preconditioner() inverts."""
    M = B.constant_operator(H, W, mask)
    return bbar / (float(dx) * float(dx)) * M + cbar * np.eye(M.shape[0])


def pcg(AC, b, rho, c, dx, mask, tol=1e-10, max_iterations=500, x0=None):
    """The device loop: PCG in the W inner product on (A + C) x = b -> (x, iterations, sqrt(sum w r^2 / sum w b^2))."""
    H, W = rho.shape
    w = B.weights(H, W, mask).ravel()
    dot = lambda a, d: float(w @ (a * d))
    minv = preconditioner(H, W, mask, dx, *means(rho, c, mask))
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - AC @ x
    bb = dot(b, b)
    it = 0
    if dot(r, r) > tol * tol * bb:
        z = minv(r)
        p, rz = z.copy(), dot(r, z)
        while it < max_iterations:
            q = AC @ p
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
    return x, it, (np.sqrt(dot(r, r) / bb) if bb > 0 else 0.0)


def face_coefficient_range(rho, mask):
    """(min, max) of beta = 2 / (rho_a + rho_b) over the faces with at least one unknown end: the faces A is made of."""
    rho = np.asarray(rho, dtype=np.float64)
    H, W = rho.shape
    i0, i1, j0, j1 = B.unknowns(H, W, mask)
    unk = np.zeros((H, W), dtype=bool)
    unk[i0:i1 + 1, j0:j1 + 1] = True
    bi, bj = 2.0 / (rho[:-1] + rho[1:]), 2.0 / (rho[:, :-1] + rho[:, 1:])
    used = np.concatenate([bi[unk[:-1] | unk[1:]], bj[unk[:, :-1] | unk[:, 1:]]])
    return float(used.min()), float(used.max())


def spectrum_bound(rho, c, mask):
    """(lo, hi): v.W(A + C)v / v.W(bbar M + cbar I)v lies in [lo, hi] for every v; c / cbar counts only where cbar > 0."""
    cbar, bbar = means(rho, c, mask)
    bmin, bmax = face_coefficient_range(rho, mask)
    lo, hi = bmin / bbar, bmax / bbar
    if cbar > 0:
        cu = on_unknowns(c, mask)
        lo, hi = min(lo, float(cu.min()) / cbar), max(hi, float(cu.max()) / cbar)
    return lo, hi
