"""CPU: the bounds of tests/bn_bounds.py have teeth.  A numpy emulation of fp32 accumulation in the kernels' summation order shows that the
one-pass formula var = E[a^2] - E[a]^2 breaks them as soon as a channel is off-centre, and that the centred scheme of csrc/pointwise.hip
(sums about the average of the channel's first pixels, backward sums about the saved mean) meets every one of them at every shape of tests/test_gpu_batchnorm.py."""
import numpy as np
import pytest

from tests import bn_bounds as B

VEC4 = {'vec4_c28': True, 'scalar_c6_16k': False, 'npix1': True, 'c256': True, 'c1': False, 'slice_aligned': True, 'slice_misaligned': False, 'ratio0': True}


def test_colsum_emulation_adds_every_element_once():
    rng = np.random.default_rng(0)
    for npix, C, vec4 in ((874, 28, True), (16384, 6, False), (1, 8, True), (15, 256, True), (189, 1, False), (300000, 4, True)):
        R, nb = B.sums_layout(npix, C, vec4)
        x = rng.integers(-8, 9, (npix, C)).astype(np.float32)         # small integers: every fp32 sum is exact in any order
        assert np.array_equal(B.fp32_colsum(x, R, nb), x.astype(np.float64).sum(0))
    assert B.sums_layout(16384, 6, False) == (32, 32) and B.sums_layout(874, 28, True) == (36, 7) and B.sums_layout(10 ** 7, 4, True)[1] == 1024


@pytest.mark.parametrize('name', sorted(B.SHAPES))
def test_centred_scheme_meets_every_bound(name):
    case = B.make_case(name)
    ref = B.reference(case)
    got = B.emulate(case, 'centred', VEC4[name])
    assert B.violations(B.forward_checks(case, ref, got)) == []
    assert B.violations(B.backward_checks(case, ref, got)) == []
    got = B.emulate(case, 'centred', VEC4[name])
    got['y'] = got['y'] + np.float32(case['residual'])
    assert B.violations(B.forward_checks(case, ref, got, residual=case['residual'])) == []


def test_naive_formula_violates_the_bounds_off_centre():
    """16384 pixels: ratio 0 passes, |ratio| >= 30 breaks the y bound and the variance (inv_std) bound; the constant channel's
    variance is not 0."""
    case = B.make_case('scalar_c6_16k')
    assert list(np.abs(case['ratio'])) == [0.0, 3.0, 30.0, 300.0, 100.0, np.inf]
    ref = B.reference(case)
    fwd = B.forward_checks(case, ref, B.emulate(case, 'naive'))
    bwd = B.backward_checks(case, ref, B.emulate(case, 'naive'))
    for c in (2, 3, 4):
        for name in ('y', 'inv_std'):
            err, bound = fwd[name]
            assert err[c] > bound[c], (name, c, err[c], bound[c])
    for name, (err, bound) in list(fwd.items()) + list(bwd.items()):
        assert err[0] <= bound[0], (name, err[0], bound[0])
    assert fwd['y'][0][5] > 0                                           # the constant channel: y != beta
    case = B.make_case('ratio0')                                        # centred channels only: the one-pass formula is good enough
    ref, got = B.reference(case), B.emulate(case, 'naive', True)
    assert B.violations(B.forward_checks(case, ref, got)) == [] and B.violations(B.backward_checks(case, ref, got)) == []
