"""Records what the four finite-difference Poisson solvers and the two seeded FD generators return, for tests/test_gpu_fd_solver_golden.py:
inputs drawn from a seeded numpy generator (rounded to fp32) and the outputs of the GPU run, in tests/golden/fd_solver_parent.npz.  Only the
Python API of poisson_cnn_amd.dataset is used, so the same file runs on any commit: the committed golden is the run of the commit BEFORE the
solvers were folded into one pipeline, and the test holds the present code to it.

    python tools/record_fd_solver_golden.py [out.npz]

The test imports `inputs`, `solve` and `generator_batches` from here, so golden and test cannot drift apart in how a case is run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fd_solver_parent.npz')
EDGES = ('left', 'right', 'bottom', 'top')
ALL_MASKS = [tuple(bool(m >> k & 1) for k in range(4)) for m in range(16)]            # (left, right, bottom, top) is Neumann
# (H, W, N) -> the solves run on that grid's one set of inputs; 9x7 carries the batch that is not a power of two
GRIDS = {
    (3, 3, 2): ['gemm'],                       # one unknown, all four edge terms
    (3, 8, 2): ['gemm'],                       # a single interior row: every unknown touches two opposite edges
    (8, 3, 2): ['gemm'],                       # ... a single interior column
    (9, 7, 3): ['gemm', 'fft', 'varcoef', 'varcoef_guess'],
    (33, 47, 2): ['gemm', 'fft', 'varcoef', 'varcoef_guess', ('mixed', (False, True, True, False)), ('mixed', (True, True, True, True))],
    (6, 5, 2): [('mixed', m) for m in ALL_MASKS],
}


def tag(kind):
    return kind if isinstance(kind, str) else 'mixed_' + ''.join('N' if f else 'D' for f in kind[1])


def inputs(H, W, N):
    """The one set of host inputs of a grid: rhs, the four edge arrays, dx, and for the variable-density solve rho in (1, 10) and a start value."""
    rng = np.random.default_rng([20, H, W, N])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = {'rhs': f32(rng.standard_normal((N, H, W))), 'dx': f32(rng.uniform(5e-3, 5e-2, N))}
    for k in EDGES:
        d[k] = f32(rng.standard_normal((N, W if k in ('left', 'right') else H)))
    d['rho'] = f32(rng.uniform(1.0, 10.0, (N, H, W)))
    d['guess'] = f32(rng.standard_normal((N, H, W)))
    return d


def solve(kind, d):
    """One solve on the GPU -> {name: numpy array}."""
    from poisson_cnn_amd import dataset as D
    from poisson_cnn_amd.dataset import _kernels as K
    dev = lambda a: torch.tensor(a, device='cuda')
    bc = {k: d[k] for k in EDGES}
    if kind in ('gemm', 'fft'):
        return {'soln': K.fd_poisson_dst(dev(d['rhs']), *[dev(d[k]) for k in EDGES], dev(d['dx']), solver=kind).cpu().numpy()}
    if kind in ('varcoef', 'varcoef_guess'):
        soln, info = D.variable_density_poisson_solve(d['rho'], d['rhs'], bc, d['dx'], tol=1e-10, return_info=True,
                                                      initial_guesses=d['guess'] if kind == 'varcoef_guess' else None)
        return dict({k: np.asarray(info[k]) for k in ('iterations', 'converged', 'relative_residual')}, soln=soln[:, 0].cpu().numpy())
    types = {k: 'neumann' if f else 'dirichlet' for k, f in zip(EDGES, kind[1])}
    return {'soln': D.mixed_bc_poisson_solve(d['rhs'], bc, d['dx'], types)[:, 0].cpu().numpy()}


def generator_batches():
    """The first two batches of the seeded generators, every tensor in the order the generator returns it, the solution last."""
    from poisson_cnn_amd import dataset as D
    gens = {
        'numerical': D.numerical_dataset_generator(batch_size=2, batches_per_epoch=2, seed=1, output_shape=[24, 20], return_boundaries=True),
        'numerical_neumann_left': D.numerical_dataset_generator(batch_size=2, batches_per_epoch=2, seed=1, output_shape=[24, 20], return_boundaries=True,
                                                                boundary_types={'left': 'neumann'}),
        'variable_density': D.variable_density_dataset_generator(batch_size=2, batches_per_epoch=2, seed=1, output_shape=(24, 20), boundaries='random'),
    }
    out = {}
    for name, gen in gens.items():
        for b in range(2):
            inp, soln = gen[b]
            for i, t in enumerate(list(inp) + [soln]):
                out['gen/%s/%d/%d' % (name, b, i)] = t.cpu().numpy()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {}
    for (H, W, N), kinds in GRIDS.items():
        d = inputs(H, W, N)
        out.update({'in/%dx%dx%d/%s' % (H, W, N, k): v for k, v in d.items()})
        for kind in kinds:
            out.update({'out/%dx%dx%d/%s/%s' % (H, W, N, tag(kind), k): v for k, v in solve(kind, d).items()})
    out.update(generator_batches())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
