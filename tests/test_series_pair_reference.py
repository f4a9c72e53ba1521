"""The numpy twin of the series pair synthesis (tests/series_pair_twin.py) has the properties the generator built on it promises, for all 16
combinations of edge types - no GPU needed.  The three bounds are the ones tests/test_gpu_dataset.py applies to the sine and cosine generators."""
import functools

import numpy as np
import pytest

from oracle import dataset as ods
from tests import series_pair_twin as T

N, H, W = 3, 120, 144


@functools.lru_cache(maxsize=None)
def inputs():
    """(coef (N,4,4) with one sample's mode counts cut to 2 x 3, dx (N,)); float32-representable, read and never written."""
    rng = np.random.default_rng(11)
    coef = rng.uniform(-1, 1, (N, 4, 4)).astype(np.float32).astype(np.float64)
    coef[1, 2:, :] = 0
    coef[1, :, 3:] = 0
    dx = rng.uniform(5e-3, 5e-2, N).astype(np.float32).astype(np.float64)
    return coef, dx


@functools.lru_cache(maxsize=None)
def pair_of(flags, dtype):
    coef, dx = inputs()
    ba, bb, wa, wb = T.bases_of(flags, 4, 4)
    return T.pair(coef, T.eigenvalues(wa, dx, H), T.eigenvalues(wb, dx, W), H, W, ba, bb, dtype=dtype)


@pytest.mark.parametrize('flags', T.all_flags(), ids=lambda f: ''.join('ND'[not v] for v in f))
def test_pair_solves_the_pde_with_its_edge_conditions(flags):
    _, dx = inputs()
    u, f = pair_of(flags, np.float64)
    res = T.pde_residual(u, f, dx)
    u32, f32 = pair_of(flags, np.float32)
    dirichlet, neumann = T.edge_defects(u32, flags)
    print('flags %s: PDE rel-L2 %.3g, Dirichlet edges %.3g, Neumann edges %.3g, fp32 restatement vs fp64 %.3g / %.3g'
          % (flags, res, dirichlet, neumann, np.linalg.norm(u32 - u) / np.linalg.norm(u), np.linalg.norm(f32 - f) / np.linalg.norm(f)))
    assert res <= 5e-2
    assert dirichlet <= 1e-5
    assert neumann <= 5e-3
    d64, n64 = T.edge_defects(u, flags)
    assert d64 <= 1e-5 and n64 <= 5e-3


def test_basis_map():
    assert [T.axis_basis(lo, hi) for lo, hi in ((0, 0), (1, 1), (0, 1), (1, 0))] == [0, 1, 2, 3]
    ba, bb, wa, wb = T.bases_of(T.neumann_flags({'left': 'neumann', 'top': 'Neumann'}), 3, 2)
    assert (ba, bb) == (3, 2) and wa.tolist() == [0.5, 1.5, 2.5] and wb.tolist() == [0.5, 1.5]
    ba, bb, wa, wb = T.bases_of((True, True, False, False), 2, 2)
    assert (ba, bb) == (1, 0) and wa.tolist() == [1.0, 2.0] and wb.tolist() == [1.0, 2.0]
    with pytest.raises(ValueError):
        T.basis(4, 2, np.zeros(3))


@pytest.mark.parametrize('kind,kw', [(0, 'sin_coeff'), (1, 'cos_coeff')])
def test_whole_wave_bases_are_the_oracle_series(kind, kw):
    rng = np.random.default_rng(kind)
    c = rng.uniform(-1, 1, (2, 5, 8))
    la, lb = rng.uniform(-9, -1, (2, 5)), rng.uniform(-9, -1, (2, 8))
    u, f = T.pair(c, la, lb, 45, 70, kind, kind)
    for n in range(2):
        assert np.allclose(u[n], ods.generate_smooth_function((45, 70), **{kw: c[n]}), rtol=0, atol=1e-12)
        assert np.allclose(f[n], ods.generate_smooth_function((45, 70), **{kw: c[n] * (la[n][:, None] + lb[n][None, :])}), rtol=0, atol=1e-11)
