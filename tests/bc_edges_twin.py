"""Twins of the per-edge boundary operators, written from their definitions (include/pcnn.h: pcnn_bc_ring_edges_fwd, pcnn_jacobi_fused_bc_fwd).

On an (N,1,H,W) tensor the edges are left: y = 0, right: y = H-1, bottom: x = 0, top: x = W-1, and neumann_mask has bit 0 / 1 / 2 / 3 set where the
left / right / bottom / top edge is Neumann.  At a corner a Dirichlet edge wins.

  E_m   the ring: interior copied; a ring point on any Dirichlet edge is 0; any other ring point is x[clamp(y,1,H-2), clamp(x,1,W-2)].
  R_m   the refresh of the smoother's frozen band of widths ry, rx: a point in no band, or in a band on a Dirichlet edge, keeps its value; any other
        band point takes the value at (my, mx): my = 2 ry - 1 - y in the left band, 2 (H-ry) - 1 - y in the right band, y otherwise; mx likewise.
  one boundary-aware sweep is R_m o J with J the oracle's sweep (np_ops.jacobi_iterations, one iteration).

Both operators are one gather `v[..., MY, MX]` (times a 0/1 map for E_m), so the same index tables serve numpy (fp64 values) and torch-CPU (adjoints by
autograd).  `recurrence` is the float32 evaluation the tolerance rule of tests/test_gpu_jacobi_stencil.py needs: the same sweeps in a chosen dtype on the
kernel's coefficient rows, forward or adjoint."""
import functools

import numpy as np
import torch

from oracle import np_ops, torch_twin

EDGES = ('left', 'right', 'bottom', 'top')


def mask_of(boundary_types):
    """dict edge -> 'dirichlet' | 'neumann' (missing: Dirichlet) -> neumann_mask."""
    return sum(1 << i for i, e in enumerate(EDGES) if str((boundary_types or {}).get(e, 'dirichlet')).lower() == 'neumann')


def bits(mask):
    return [bool(mask >> i & 1) for i in range(4)]


@functools.lru_cache(maxsize=None)
def tables(H, W, mask, ry, rx):
    """(MY, MX, frozen): for every point where its value comes from - itself unless R_m refreshes it - and whether it lies in a band on a Dirichlet edge.
    Cached: read, never written."""
    nl, nr, nb, nt = bits(mask)
    MY, MX = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    MY, MX = MY.copy(), MX.copy()
    frozen = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            my, mx, dirichlet = y, x, False
            if y < ry:
                my, dirichlet = (2 * ry - 1 - y, dirichlet) if nl else (y, True)
            elif y >= H - ry:
                my, dirichlet = (2 * (H - ry) - 1 - y, dirichlet) if nr else (y, True)
            if x < rx:
                mx, dirichlet = (2 * rx - 1 - x, dirichlet) if nb else (x, True)
            elif x >= W - rx:
                mx, dirichlet = (2 * (W - rx) - 1 - x, dirichlet) if nt else (x, True)
            if dirichlet:
                my, mx = y, x
            MY[y, x], MX[y, x], frozen[y, x] = my, mx, dirichlet
    return MY, MX, frozen


def _gather(v, MY, MX):
    if isinstance(v, torch.Tensor):
        return v[..., torch.as_tensor(MY), torch.as_tensor(MX)]
    return np.asarray(v)[..., MY, MX]


def ring(x, mask):
    """E_m x, numpy or torch, (..., H, W)."""
    H, W = x.shape[-2:]
    MY, MX, frozen = tables(H, W, mask, 1, 1)
    keep = (~frozen).astype(np.float64)
    return _gather(x, MY, MX) * (torch.as_tensor(keep, dtype=x.dtype) if isinstance(x, torch.Tensor) else keep)


def refresh(v, mask, ss):
    """R_m v."""
    H, W = v.shape[-2:]
    MY, MX, _ = tables(H, W, mask, ss[0] // 2, ss[1] // 2)
    return _gather(v, MY, MX)


def sweeps(u, rhs, dx, n, mask, ss=(3, 3), od=(2, 2)):
    """(R_m J)^n u in fp64 numpy; u, rhs (N,1,H,W), dx (N,2)."""
    x = np.asarray(u, dtype=np.float64)
    for _ in range(n):
        x = refresh(np_ops.jacobi_iterations(x, rhs, dx, 1, ss, od), mask, ss)
    return x


def sweeps_torch(u, rhs, dx, n, mask, ss=(3, 3), od=(2, 2)):
    """The same on torch-CPU fp64 tensors, differentiable w.r.t. u."""
    x = u
    for _ in range(n):
        x = refresh(torch_twin.jacobi_iterations(x, rhs, dx, 1, ss, od), mask, ss)
    return x


def adjoint(u_shape_like, rhs, dx, dout, n, mask, ss=(3, 3), od=(2, 2)):
    """(J^T R_m^T)^n dout by autograd through sweeps_torch (the operator is affine in u: any u gives the same adjoint)."""
    ut = torch.zeros(np.asarray(u_shape_like).shape, dtype=torch.float64, requires_grad=True)
    (sweeps_torch(ut, rhs, dx, n, mask, ss, od) * torch.as_tensor(np.asarray(dout), dtype=torch.float64)).sum().backward()
    return ut.grad.numpy().copy()


def ring_adjoint(w, mask):
    """E_m^T w by autograd."""
    v = torch.zeros(np.asarray(w).shape, dtype=torch.float64, requires_grad=True)
    (ring(v, mask) * torch.as_tensor(np.asarray(w), dtype=torch.float64)).sum().backward()
    return v.grad.numpy().copy()


def recurrence(x, rhs, rows, ss, n, mask, dtype, adjoint=False):
    """n boundary-aware sweeps (or adjoint sweeps) in `dtype` numpy on the kernel's coefficient rows (N, sy+sx+1): the H taps, the W taps, 1 / diagonal.
    The taps are summed in the kernel's order, without fused multiply-adds."""
    sy, sx = ss
    ry, rx = sy // 2, sx // 2
    x = np.asarray(x, dtype=dtype)[:, 0]
    rhs = np.asarray(rhs, dtype=dtype)[:, 0]
    rows = np.asarray(rows, dtype=dtype)
    Nn, H, W = x.shape
    MY, MX, _ = tables(H, W, mask, ry, rx)
    inner = np.zeros((H, W), dtype=dtype)
    inner[ry:H - ry, rx:W - rx] = 1
    dinv = rows[:, sy + sx][:, None, None]
    for _ in range(n):
        if adjoint:                                             # R_m^T: every point hands its gradient to the point its value came from
            g = np.zeros_like(x)
            for b in range(Nn):
                np.add.at(g[b], (MY, MX), x[b])
            x = g.astype(dtype)
        src = x * inner if adjoint else x                       # J^T gathers from interior points only
        p = np.zeros((Nn, H + 2 * ry, W + 2 * rx), dtype=dtype)
        p[:, ry:ry + H, rx:rx + W] = src
        acc = np.zeros_like(x)
        for i in range(sy):
            if i != ry:
                o = (i - ry) * (-1 if adjoint else 1)
                acc = acc + rows[:, i][:, None, None] * p[:, ry + o:ry + o + H, rx:rx + W]
        for j in range(sx):
            if j != rx:
                o = (j - rx) * (-1 if adjoint else 1)
                acc = acc + rows[:, sy + j][:, None, None] * p[:, ry:ry + H, rx + o:rx + o + W]
        if adjoint:
            x = (x * (1 - inner) - dinv * acc).astype(dtype)
        else:
            x = (inner * (dinv * (rhs - acc)) + (1 - inner) * x).astype(dtype)
            x = x[:, MY, MX]
    return x[:, None].astype(np.float64)
