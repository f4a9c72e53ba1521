"""Homogeneous_Poisson_NN_Legacy(density_input=True).solve: the variable-density conjugate-gradient solve started from the model's prediction.  The
tiny model and the 2 x 24 x 28 batch of tests/test_gpu_varcoef_model.py; the reference is the direct sparse fp64 solve of tests/varcoef_twin.py."""
import functools

import numpy as np
import pytest
import torch

from tests import error_stats_twin as ST, test_gpu_varcoef_model as VM, varcoef_twin as VT

pytestmark = pytest.mark.gpu
N, H, W = VM.N, VM.H, VM.W
TOL_F32 = 2e-7             # rel-L2 of an fp32 solution against the fp64 twin: the bound of tests/test_gpu_varcoef.py
EPS = 2.0 ** -23
# prediction_relative_residual = sqrt(sum r^2 / sum f^2) against the float32-term twin.  Each sum is off by at most (chain + 1) eps relative
# (tests/test_gpu_varcoef_stats.py): at 24 x 28 one addition per lane, 6 + 15 + 6 in the tree, one rounding for the square: 29 eps.  The ratio of
# the two sums is off by twice that and the square root halves it again.
TOL_RESIDUAL = 29 * EPS


@functools.lru_cache(maxsize=None)
def problem():
    """(stack, dx, rho, rhs, zero edges, the twin's solution (N,H,W) in fp64) - computed once, never written to"""
    stack, dx, _ = VM.batch()
    rhs, rho = stack[:, 0], stack[:, 1]
    zero = {'left': np.zeros((N, W)), 'right': np.zeros((N, W)), 'bottom': np.zeros((N, H)), 'top': np.zeros((N, H))}
    return stack, dx, rho, rhs, zero, VT.solve_batch(rho, rhs, zero, dx[:, 0])


@functools.lru_cache(maxsize=None)
def model():
    return VM.build(VM.model_cfg(2, density_input=True))[0]


def test_warm_and_cold_solves_match_the_fp64_twin():
    from poisson_cnn_amd import dataset as D
    stack, dx, rho, rhs, zero, ref = problem()
    m = model()
    warm, info = m.solve([stack, dx], return_info=True)
    cold, info_cold = m.solve([stack, dx], warm_start=False, return_info=True)
    assert tuple(warm.shape) == (N, 1, H, W) and warm.dtype == torch.float32 and info['converged'].all() and info_cold['converged'].all()
    for name, s, i in (('warm', warm, info), ('cold', cold, info_cold)):
        err = VM.rel(s.cpu().numpy()[:, 0], ref)
        print('%s start: rel-L2 vs the fp64 twin %.3g, iterations %r, prediction residual %r' % (name, err, i['iterations'].tolist(),
                                                                                                 i['prediction_relative_residual'].tolist()))
        assert err <= TOL_F32
    assert torch.equal(m.solve([stack, dx]), warm)                                         # without return_info: the tensor alone
    # the warm result is the public solver's, started at the model's own output
    direct = D.variable_density_poisson_solve(rho, rhs, zero, dx, initial_guesses=m([stack, dx]))
    assert torch.equal(warm, direct)
    assert torch.equal(cold, D.variable_density_poisson_solve(rho, rhs, zero, dx))


def test_prediction_residual_is_the_twins_on_the_models_own_output():
    stack, dx, rho, rhs, _, _ = problem()
    m = model()
    _, info = m.solve([stack, dx], return_info=True)
    pred = m([stack, dx]).cpu().numpy()
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    tw = ST.error_stats(pred, None, f32(rhs), f32(dx[:, 0]), f32(rho), float32_terms=True)
    want = np.sqrt(tw[:, 5] / tw[:, 7])
    got = info['prediction_relative_residual']
    print('prediction_relative_residual %r, twin %r, error / bound %.3g' % (got.tolist(), want.tolist(), (np.abs(got - want) / want).max() / TOL_RESIDUAL))
    assert got.shape == (N,) and np.all(np.abs(got - want) <= TOL_RESIDUAL * want)
    # r is formed in the twin's float32 order, so the maximum is the same float32 number
    assert np.array_equal(info['prediction_max_residual'], tw[:, 6])


def test_a_start_at_the_solution_needs_no_iteration():
    """The forward replaced by the twin's solution (fp64, as the solver reads its start): the start already meets tol."""
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    stack, dx, _, _, _, ref = problem()

    class Exact(Homogeneous_Poisson_NN_Legacy):
        def call(self, inp, training=False):
            return torch.tensor(ref[:, None], dtype=torch.float64, device=self.device)

    m = Exact(**VM.model_cfg(2, density_input=True))
    soln, info = m.solve([stack, dx], return_info=True, compare_cold=True, check_every=4)
    assert (info['iterations'] == 0).all() and info['converged'].all()
    assert torch.equal(soln.cpu(), torch.tensor(ref[:, None], dtype=torch.float32))        # the embedded start: interior in fp32, zero edges
    assert np.all(np.isfinite(info['prediction_relative_residual']))                        # of the fp32-rounded solution, in fp32 arithmetic
    print('fp32 residual of the rounded solution: %r' % info['prediction_relative_residual'].tolist())
    assert np.all(info['cold_iterations'] > 0) and np.all(info['cold_iterations'] % 4 == 0)


def test_compare_cold_reports_the_cold_solves_iterations():
    stack, dx, _, _, _, _ = problem()
    m = model()
    _, info = m.solve([stack, dx], return_info=True, compare_cold=True, check_every=4)
    _, cold = m.solve([stack, dx], return_info=True, compare_cold=True, check_every=4, warm_start=False)
    assert 'cold_iterations' not in m.solve([stack, dx], return_info=True)[1]
    assert info['cold_iterations'].shape == (N,) and np.all(info['cold_iterations'] > 0) and np.all(info['cold_iterations'] % 4 == 0)
    assert np.array_equal(cold['cold_iterations'], cold['iterations']) and np.array_equal(cold['iterations'], info['cold_iterations'])
    print('iterations warm %r, cold %r' % (info['iterations'].tolist(), info['cold_iterations'].tolist()))
    assert np.all(info['iterations'] % 4 == 0)
    nan = m.solve([np.concatenate([0 * stack[:, :1], stack[:, 1:]], 1), dx], warm_start=False, return_info=True)[1]      # rhs = 0: no relative residual
    assert np.isnan(nan['prediction_relative_residual']).all() and nan['converged'].all()


def test_solve_leaves_the_model_as_it_was():
    from poisson_cnn_amd.losses import variable_density_loss_wrapper
    from poisson_cnn_amd.train import Adam
    stack, dx, _, _, _, _ = problem()
    m = VM.build(VM.model_cfg(2, density_input=True))[0]
    m.compile(loss=variable_density_loss_wrapper(global_batch_size=N, **VM.loss_params(1e-9)), optimizer=Adam(learning_rate=1e-3))
    m.train_step(((stack, dx), VM.batch()[2]))                                              # moments and a step count that are not zero
    opt = m.optimizer
    state = lambda: [m.store.flat_w, m.store.flat_stats, m.store.flat_g] + list(opt.ms) + list(opt.vs)
    before, steps = [t.clone() for t in state()], opt.iterations
    assert steps == 1 and float(opt.ms[0].abs().max()) > 0
    m.solve([stack, dx], return_info=True, compare_cold=True)
    assert opt.iterations == steps
    for a, b in zip(before, state()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_refusals():
    from poisson_cnn_amd.models import Homogeneous_Poisson_NN_Legacy
    stack, dx, _, _, _, _ = problem()
    plain = Homogeneous_Poisson_NN_Legacy(**VM.model_cfg(0))
    with pytest.raises(ValueError, match=r'dataset\.multigrid_poisson_solve'):
        plain.solve([stack[:, :1], dx])
    m = model()
    with pytest.raises(NotImplementedError, match='anisotropic'):
        m.solve([stack, np.concatenate([dx, 2 * dx], 1)])
    assert torch.equal(m.solve([stack, np.concatenate([dx, dx], 1)]), m.solve([stack, dx]))      # equal columns are one spacing
    with pytest.raises(ValueError, match=r'\(N,2,H,W\)'):
        m.solve([stack[:, :1], dx])
