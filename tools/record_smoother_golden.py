"""Records what the Jacobi smoothers, the residual losses and error_stats return, for tests/test_gpu_smoother_golden.py: inputs drawn from a
seeded numpy generator (rounded to fp32) and the outputs of the GPU run, in tests/golden/smoother_parent.npz.  Only poisson_cnn_amd.ops is used,
so the same file runs on any commit: the committed golden is the run of the commit BEFORE the two smoother families were put on one sweep driver
(csrc/sweep_common.h), and the test holds the present code to it bit for bit.

    python tools/record_smoother_golden.py [out.npz]

The test imports `CASES`, `inputs`, `run` and `stored` from here, so golden and test cannot drift apart in how a case is run.

An array of more than FULL_MAX elements (the 65 x 130 fields; the case list has about a hundred of them, 68 KB each) is stored as the SHA-256 of its
dtype, shape and bytes instead of its values: equal digests are equal bits, and the file stays well under the size limit of a committed file.  Smaller
arrays are stored as they are, and so are the 65 x 130 outputs of the FULL cases - the chain of three launches of each sweep family - so that a
difference there can be located."""
import functools
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'smoother_parent.npz')
FULL_MAX = 4096

FUSED_STENCILS = {(3, 3): 8, (5, 3): 4, (9, 9): 2}                  # stencil -> the k_max the case list was written for (the test checks it)
FUSED_GRIDS = [(9, 9), (3, 70), (70, 3), (65, 130)]                  # 3 x 70 and 70 x 3: one interior line, (3, 3) only; (9, 9) needs H, W >= 9
MASK_GRIDS = [(13, 13), (65, 130)]
MASKS = [0, 5, 15]
VARCOEF_K_MAX = 8
VARCOEF_SWEEPS = [1, 8, 9, 17]
VARCOEF_GRIDS = [(3, 3), (3, 70), (70, 3), (65, 130)]
LOSS_GRIDS = [(3, 3), (18, 66), (19, 67), (35, 131)]                 # interior: one node, exactly one 16 x 64 tile, one over in both axes, several tiles


def sweep_counts(k):
    return [1, k, k + 1, 2 * k + 1]           # one launch; one full launch; a chain of two, uneven; a chain of three (out / scratch parity)


def _cases():
    c = []
    for ss, k in FUSED_STENCILS.items():
        for H, W in FUSED_GRIDS:
            if min(H, W) == 3 and ss != (3, 3) or H < ss[0] or W < ss[1]:
                continue
            c += [('fused', ss, (H, W, 2), n, 0) for n in sweep_counts(k)]
        for H, W in MASK_GRIDS:
            c += [('fused', ss, (H, W, 2), n, m) for m in MASKS for n in sweep_counts(k) if ('fused', ss, (H, W, 2), n, m) not in c]   # mask 0 on 65 x 130 is above
    c += [('sweep', (3, 3), (H, W, 2), 1, 0) for H, W in ((3, 3), (65, 130))]
    c += [('varcoef', (3, 3), (H, W, 2), n, 0) for H, W in VARCOEF_GRIDS for n in VARCOEF_SWEEPS]
    c += [('varcoef_loss', (3, 3), (H, W, 3), 0, 0) for H, W in LOSS_GRIDS]
    c += [('pi_loss', ss, (19, 67, 3), 0, 0) for ss in ((3, 3), (5, 3))]
    c += [('error_stats', (3, 3), (19, 67, 3), 0, 0)]
    return c


CASES = _cases()                              # (kind, stencil, (H, W, N), sweeps, neumann mask)
FULL = [('fused', (3, 3), (65, 130, 2), 17, 15), ('varcoef', (3, 3), (65, 130, 2), 17, 0)]      # their outputs are stored as values whatever their size


def case_id(case):
    kind, ss, (H, W, N), n, m = case
    return '%s/%dx%d/%dx%dx%d/n%d/m%d' % (kind, ss[0], ss[1], H, W, N, n, m)


def stored(a, full=False):
    """The form an array takes in the golden file."""
    a = np.ascontiguousarray(a)
    if full or a.size <= FULL_MAX:
        return a
    return np.frombuffer(hashlib.sha256(('%s%s' % (a.dtype.str, a.shape)).encode() + a.tobytes()).digest(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(H, W, N):
    """The one set of host inputs of a grid, shared by every case on it: read, never written."""
    rng = np.random.default_rng([21, H, W, N])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = {k: f32(rng.standard_normal((N, H, W))) for k in ('u', 'rhs', 'dout', 'target', 'dpred')}
    d['rho'] = f32(rng.uniform(1.0, 10.0, (N, H, W)))
    d['dx2'] = f32(rng.uniform(5e-3, 5e-2, (N, 2)))                  # a different spacing per sample and per axis
    d['lcoef'] = f32(rng.uniform(0.5, 2.0, N))
    # tap weights of a 9-point line per axis; a stencil takes its middle entries.  Positive taps over their negated sum: a sweep averages, so no
    # sweep count overflows
    d['wy'], d['wx'] = f32(rng.uniform(0.5, 1.5, 9)), f32(rng.uniform(0.5, 1.5, 9))
    return d


def stencil(d, ss):
    """Per sample: the H taps, the W taps (centres zero) and the diagonal of a cross-shaped operator with d's spacings."""
    sy, sx = ss
    ty = np.array(d['wy'][4 - sy // 2: 5 + sy // 2]); ty[sy // 2] = 0
    tx = np.array(d['wx'][4 - sx // 2: 5 + sx // 2]); tx[sx // 2] = 0
    cy = (ty[None, :] / d['dx2'][:, 0:1] ** 2).astype(np.float32)
    cx = (tx[None, :] / d['dx2'][:, 1:2] ** 2).astype(np.float32)
    diag = -(cy.sum(axis=1) + cx.sum(axis=1)).astype(np.float32)
    return cy, cx, diag


def run(case, d):
    """One case on the GPU -> {name: numpy array}."""
    from poisson_cnn_amd import ops
    kind, ss, (H, W, N), n, mask = case
    dev = lambda a: torch.tensor(a, device='cuda')
    nhw1 = lambda a: dev(a[..., None])
    host = lambda t: t.cpu().numpy().reshape(N, H, W)
    if kind == 'fused':
        cy, cx, diag = stencil(d, ss)
        coef = dev(np.ascontiguousarray(np.concatenate([cy, cx, (1.0 / diag)[:, None]], axis=1), dtype=np.float32))
        return {'fwd': host(ops.jacobi_fused(nhw1(d['u']), nhw1(d['rhs']), coef, ss, n, mask)),
                'bwd': host(ops.jacobi_fused_bwd(nhw1(d['dout']), coef, ss, n, mask))}
    if kind == 'sweep':
        return {'fwd': host(ops.jacobi_sweep(nhw1(d['u']), nhw1(d['rhs']), dev(d['dx2']))),
                'bwd': host(ops.jacobi_sweep_bwd(nhw1(d['dout']), dev(d['dx2'])))}
    dx = dev(np.ascontiguousarray(d['dx2'][:, 0]))
    if kind == 'varcoef':
        return {'fwd': host(ops.varcoef_jacobi(dev(d['u']), dev(d['rho']), dev(d['rhs']), dx, n)),
                'bwd': host(ops.varcoef_jacobi_bwd(dev(d['dout']), dev(d['rho']), dx, n))}
    if kind == 'varcoef_loss':
        pred, rho, rhs = dev(d['u']), dev(d['rho']), dev(d['rhs'])
        return {'sums': ops.varcoef_pi_loss_partials(pred, rho, rhs, dx).cpu().numpy(),
                'dpred': host(ops.varcoef_pi_loss_bwd(pred, rho, rhs, dx, dev(d['lcoef']), dev(d['dpred'])))}     # accumulates into a non-zero dpred
    if kind == 'pi_loss':
        cy, cx, diag = stencil(d, ss)
        kern = np.zeros((N,) + tuple(ss), dtype=np.float32)
        kern[:, :, ss[1] // 2] = cy
        kern[:, ss[0] // 2, :] = cx
        kern[:, ss[0] // 2, ss[1] // 2] = diag
        pred, rhs, kern = dev(d['u']), dev(d['rhs']), dev(kern)
        return {'sums': ops.pi_loss_partials(pred, rhs, kern).cpu().numpy(),
                'dpred': host(ops.pi_loss_bwd(pred, rhs, kern, dev(d['lcoef']), dev(d['dpred'])))}
    assert kind == 'error_stats'
    return {'stats': ops.error_stats(dev(d['u']), dev(d['target']), dev(d['rhs']), dev(d['dx2'])).cpu().numpy()}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {}
    for case in CASES:
        H, W, N = case[2]
        d = inputs(H, W, N)
        out.update({'in/%dx%dx%d/%s' % (H, W, N, k): stored(v) for k, v in d.items()})
        out.update({'out/%s/%s' % (case_id(case), k): stored(v, case in FULL) for k, v in run(case, d).items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print('wrote %s: %d cases, %d arrays, %d bytes' % (path, len(CASES), len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
