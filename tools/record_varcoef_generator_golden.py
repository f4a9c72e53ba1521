"""Records the first batch of dataset.variable_density_dataset_generator at a fixed seed, for tests/test_gpu_varcoef_reaction.py: the two-channel
stack, the four edge arrays, dx and the solution, all Dirichlet and all Neumann, in tests/golden/varcoef_generator_parent.npz.  Only the generator's
arguments of before the reaction term are used, so the same file runs on any commit: the committed golden is the run of the commit BEFORE the
generator learnt `reaction_range`, and the test holds the present generator with reaction_range = None to it bit for bit.

    python tools/record_varcoef_generator_golden.py [out.npz]

The test imports `KW`, `CASES` and `run` from here, so golden and test cannot drift apart in how a batch is drawn."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'varcoef_generator_parent.npz')
EDGES = ('left', 'right', 'bottom', 'top')
KW = dict(batch_size=2, batches_per_epoch=1, output_shape=(33, 47), density_range=(1.0, 10.0), rhs_smoothness_range=(4, 7), density_smoothness_range=(3, 6),
          boundaries='random', seed=9)
CASES = {'dirichlet': None, 'neumann': {k: 'neumann' for k in EDGES}}
NAMES = ('stack', 'left', 'top', 'right', 'bottom', 'dx', 'soln')


def run(case, **extra):
    """The first batch of a fresh generator -> {name: host array}; extra: keywords a later commit added."""
    from poisson_cnn_amd import dataset as D
    inp, soln = D.variable_density_dataset_generator(boundary_types=CASES[case], **KW, **extra)[0]
    return {k: v.cpu().numpy() for k, v in zip(NAMES, list(inp) + [soln])}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    out = {'%s/%s' % (case, k): v for case in CASES for k, v in run(case).items()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
