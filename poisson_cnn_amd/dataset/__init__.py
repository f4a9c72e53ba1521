"""On-device reference-solution generators: drop-ins for poisson_CNN/dataset/generators (reference paths relative to
poisson_CNN/).  Same constructor kwargs (the "dataset" section of experiments/hpnn*.json loads unchanged) and the Keras
Sequence protocol: `len(gen)`, `gen[idx] -> ([rhs, (boundaries...), dx], soln)`, every tensor a float32 CUDA tensor in the
reference's channels_first layout.

  numerical_dataset_generator                              <- dataset/generators/numerical.py:152-216 (+ numerical_dataset :74-150)
  reverse_poisson_dataset_generator                        <- dataset/generators/reverse.py:101-330
  reverse_poisson_dataset_generator_homogeneous_neumann    <- dataset/generators/reverse_neumann.py:9-66

Only the O(10)-sized random parameters (shapes, spacings, coefficient grids, polynomial roots, control points) are drawn on
the host (numpy Generator seeded with `seed`; the reference's TF RNG stream cannot be reproduced, so parity is
distributional for the random draws and exact for everything computed from them); every H x W field is synthesised,
solved and normalised on the GPU.
"""
import math

import numpy as np
import torch

from . import _kernels as K
from .. import ops
from ..utils import neumann_flags


# ----------------------------------------------------------------------------- host-side samplers (dataset/utils)
def _integrate_piecewise_sigmoid(L1, L2):
    """dataset/utils/generate_uniformly_distributed_aspect_ratios.py:4-23."""
    pre = np.maximum((L2[..., 0] - L1[..., 0]) * L2[..., 0], 0.0)
    post = np.maximum((L1[..., 1] - L2[..., 1]) * L2[..., 1], 0.0)
    lo = np.maximum(L2[..., 0], L1[..., 0])
    hi = np.minimum(L2[..., 1], L1[..., 1])
    return pre + post + 0.5 * (hi ** 2 - lo ** 2)


def generate_uniformly_distributed_aspect_ratios(output_shape_range, dx_range=None, samples=1, rng=None):
    """dataset/utils/generate_uniformly_distributed_aspect_ratios.py:59-85 -> (samples, ndims-1)."""
    rng = rng or np.random.default_rng()
    osr = np.asarray(output_shape_range, dtype=np.float64)
    if dx_range is None:
        dsr = osr - 1.0
    else:
        dxr = np.asarray(dx_range, dtype=np.float64)
        dsr = np.stack([(osr[:, 0] - 1) * dxr[:, 0], (osr[:, 1] - 1) * dxr[:, 1]], -1)
    max_ar = dsr[0, 1] / dsr[1:, 0]
    min_ar = dsr[0, 0] / dsr[1:, 1]
    L1 = np.tile(dsr[0][None], (dsr.shape[0] - 1, 1))
    L2 = dsr[1:]
    prop = (L2[:, 1] * (L1[:, 1] - L1[:, 0]) - _integrate_piecewise_sigmoid(L1, L2)) / ((L2[:, 1] - L2[:, 0]) * (L1[:, 1] - L1[:, 0]))
    under = (rng.uniform(size=(samples, prop.shape[0])) < prop[None]).astype(np.float64)
    ub = min(float(np.min(max_ar)), 1.0)
    lb = max(float(np.max(min_ar)), 1.0)
    u = rng.uniform(size=under.shape)
    return under * ((ub - min_ar) * u + min_ar) + (1 - under) * ((max_ar - lb) * u + lb)


def generate_output_shapes_and_grid_spacings_from_aspect_ratios(aspect_ratios, random_output_shape_range, random_dx_range, constant_dx=False,
                                                                samples=None, rng=None):
    """dataset/utils/generate_output_shapes_and_grid_spacings_from_aspect_ratios.py:4-41 -> (npts (ndims,), dx (samples, ndims))."""
    rng = rng or np.random.default_rng()
    ar = np.asarray(aspect_ratios, dtype=np.float64)
    ndims = ar.shape[1] + 1
    osr = np.asarray(random_output_shape_range, dtype=np.int64)
    dxr = np.asarray(random_dx_range, dtype=np.float64)
    nx_min, nx_max = osr[0, 0] - 0.4999999999, osr[0, 1] + 0.4999999999
    nx = int(np.round(rng.uniform() * (nx_max - nx_min) + osr[0, 0]))
    if constant_dx:
        dx = np.tile(rng.uniform(size=(samples, 1)) * (dxr[0, 1] - dxr[0, 0]) + dxr[0, 0], (1, ndims))
        other = (nx / ar[0]).astype(np.int64)
    else:
        dx0 = (dxr[0, 1] - dxr[0, 0]) * rng.uniform(size=(ar.shape[0], 1)) + dxr[0, 0]
        Lx = (nx - 1) * dx0[:, 0]
        L = np.concatenate([np.ones((ar.shape[0], 1)), ar], -1) * Lx[:, None]
        other = (rng.uniform(size=(ndims - 1,)) * (osr[1:, 1] - osr[1:, 0])).astype(np.int64) + osr[1:, 0]
        dx = np.concatenate([dx0, L[:, 1:] / (other - 1)[None]], 1)
    npts = np.concatenate([[nx], other]).astype(np.float64)
    maxpts, minpts = osr.max(1), osr.min(1)
    over = max(1.0, float(np.max(npts / maxpts)))
    under = min(1.0, float(np.min(npts / minpts)))
    scale = over if over > 1.0 else max(under, float(np.max(npts / maxpts)))
    return (npts / scale).astype(np.int64), dx


def _range2(value_range, ndims):
    """handle_grid_parameters_range (dataset/generators/reverse.py:10-21)."""
    v = np.asarray(value_range, dtype=np.float64)
    if v.ndim == 1:
        assert v[0] <= v[1], 'Upper bound must be larger than or equal to the lower bound!'
        v = np.tile(v[None], (ndims, 1))
    assert v.shape == (ndims, 2) and np.all(v[:, 1] >= v[:, 0]) and np.all(v[:, 0] >= 0)
    return v


def _process_normalizations(n):
    """dataset/generators/reverse.py:23-36."""
    out = {'rhs_max_magnitude': False, 'max_domain_size_squared': False, 'soln_max_magnitude': False}
    if isinstance(n, dict):
        out.update(n)
        if isinstance(out['rhs_max_magnitude'], bool) and out['rhs_max_magnitude']:
            out['rhs_max_magnitude'] = 1.0
    return out


def _poly_and_second_derivative(roots, x):
    """p(x) = prod_r (x + roots[r]) and d2p/dx2 on the points x.  The reference differentiates the product twice with tf.gradients and
    patches the NaNs that produces wherever a factor vanishes (dataset/generators/reverse.py:39-71); here the product is expanded once
    (degree <= ~12, roots in [-1, 0]: exact to ~1e-13 in float64) and both are Horner evaluations - no patch, no per-pair products."""
    from numpy.polynomial import polynomial as npoly
    c = npoly.polyfromroots(-np.asarray(roots, dtype=np.float64))
    return npoly.polyval(x, c), (npoly.polyval(x, npoly.polyder(c, 2)) if c.shape[0] > 2 else np.zeros_like(x))


def _streams(seed, shard):
    """The generators' two host-side random streams.  `shard` = (rank, world_size) of a data-parallel run: the SHAPE stream - everything
    that decides the grid size (H, W) of a step, drawn for the global batch as the reference's single generator does
    (dataset/generators/reverse.py:192-193: one shape per batch, which MirroredStrategy then splits) - is seeded identically on every rank;
    the DATA stream (coefficients, control points, magnitudes) is seeded `seed + rank`.  Without a shard both are ONE stream (single process)."""
    if shard is None:
        rng = np.random.default_rng(seed)
        return rng, rng, (0, 1)
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError('shard = (rank, world_size) with 0 <= rank < world_size, got %r' % (shard,))
    return np.random.default_rng(seed + rank), np.random.default_rng([int(seed), 0x5AFE]), (rank, world)


_BOUNDARY_KEYS = ('left', 'top', 'right', 'bottom')


_neumann_flags = neumann_flags                    # (left, right, bottom, top): the one parser of boundary types, utils.neumann_flags


class _generator:
    """What every generator family shares: the Keras Sequence length and the upload of host draws to self.device."""

    def __len__(self):
        return self.batches_per_epoch

    def _dev(self, a):
        """host array -> float32 device tensor through a pinned staging buffer and an asynchronous copy on the current stream: a pageable upload
        (torch.tensor(..., device=...)) synchronises the stream, ten times per batch (profiles/r06_train_shipped.txt); torch's pinned-memory cache
        keeps the staging buffer alive until the copy has run."""
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        if self.device.type != 'cuda':
            return t.to(self.device)
        return t.pin_memory().to(self.device, non_blocking=True)

    # -- draws and fields more than one family uses (self.rng, self.batch_size, self.device and the named attributes are the subclass')
    def _grid_sizes(self, rng_range):
        """generate_grid_sizes (reverse.py:164-171)."""
        return ((rng_range[:, 1] - rng_range[:, 0]) * self.rng.uniform(size=(2,)) + rng_range[:, 0] + 1).astype(np.int64)

    def _draw_mode_counts(self):
        """Mode counts per sample and axis from self.fourier_coeff_grid_size_range -> (N,2)."""
        return np.stack([self._grid_sizes(self.fourier_coeff_grid_size_range) for _ in range(self.batch_size)])

    def _draw_coefficients(self, ncoef):
        """Series coefficients uniform in [-1, 1), zero beyond a sample's own mode counts -> (N,ka,kb), ka / kb the batch's largest counts."""
        N = self.batch_size
        ka, kb = int(ncoef[:, 0].max()), int(ncoef[:, 1].max())
        coef = np.zeros((N, ka, kb))
        for b in range(N):
            coef[b, :ncoef[b, 0], :ncoef[b, 1]] = 2 * self.rng.uniform(size=(ncoef[b, 0], ncoef[b, 1])) - 1
        return coef

    def _smooth_field(self, ctrl, out_hw, max_magnitude):
        """generate_random_RHS / generate_random_boundaries core (numerical.py:10-72): control points -> legacy bicubic
        (align_corners) up-sampling -> per-sample max-magnitude scaling."""
        N = ctrl.shape[0]
        x = self._dev(ctrl).view(N, ctrl.shape[1], ctrl.shape[2], 1)
        y = K.resize_legacy_bicubic(x, out_hw).view(N, out_hw[0], out_hw[1])
        if max_magnitude != np.inf:
            K.set_max_magnitude(y, torch.full((N,), float(max_magnitude), device=self.device))
        return y

    def _density_field(self, ctrl, out_hw):
        """rho (N,H,W) in self.density_range from control points, by self.density_profile ('abs': kinked, 'smooth'; VARIABLE_DENSITY_PROFILES)."""
        density = K.varcoef_density_smooth if self.density_profile == 'smooth' else K.varcoef_density
        return density(self._smooth_field(ctrl, out_hw, 1.0), *self.density_range)


# ----------------------------------------------------------------------------- analytic ("reverse") generators
class reverse_poisson_dataset_generator(_generator):
    def __init__(self, batch_size, batches_per_epoch, random_output_shape_range, fourier_coeff_grid_size_range, taylor_degree_range=None,
                 grid_spacings_range=None, ndims=None, homogeneous_bc=False, return_rhses=True, return_boundaries=True, return_dx=True,
                 normalizations=None, uniform_grid_spacing=False, seed=0, device=None, shard=None):
        self.batch_size, self.batches_per_epoch = int(batch_size), int(batches_per_epoch)
        self.ndims = 2 if ndims is None else ndims
        if self.ndims != 2:
            raise NotImplementedError('2-D only')
        self.homogeneous_bc = homogeneous_bc
        self.grid_spacings_range = _range2(grid_spacings_range, 2)
        self.random_output_shape_range = _range2(random_output_shape_range, 2).astype(np.int64)
        self.fourier_coeff_grid_size_range = _range2(fourier_coeff_grid_size_range, 2)
        self.taylor_degree_range = _range2(taylor_degree_range, 2) if taylor_degree_range is not None else None
        self.return_rhses, self.return_boundaries, self.return_dx = return_rhses, return_boundaries, return_dx
        self.normalizations = _process_normalizations(normalizations)
        self.uniform_grid_spacing = uniform_grid_spacing
        self.rng, self.shape_rng, self.shard = _streams(seed, shard)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.neumann = False
        self.fixed_output_shape = None     # set to (H, W) to pin the grid (benchmarks / data-parallel ranks sharing one shape)

    # -- host-side draws
    def _shape_and_spacings(self):
        """generate_grid_sizes_and_spacings_with_uniform_AR (reverse.py:173-177)."""
        # one draw for the GLOBAL batch from the stream every rank shares (one grid shape per step on all replicas, reverse.py:192-193);
        # a rank keeps its own rows of the per-sample spacings
        rank, world = self.shard
        gb = self.batch_size * world
        ar = generate_uniformly_distributed_aspect_ratios(self.random_output_shape_range, None if self.uniform_grid_spacing else self.grid_spacings_range,
                                                          gb, self.shape_rng)
        shape, dx = generate_output_shapes_and_grid_spacings_from_aspect_ratios(ar, self.random_output_shape_range, self.grid_spacings_range,
                                                                                constant_dx=self.uniform_grid_spacing, samples=gb, rng=self.shape_rng)
        dx = dx[rank * self.batch_size:(rank + 1) * self.batch_size]
        if self.fixed_output_shape is not None:
            shape = np.asarray(self.fixed_output_shape, dtype=np.int64)
        return shape, dx

    def _taylor_tables(self, H, W, domain_sizes):
        """1-D tables of generate_soln_and_rhs_taylor (reverse.py:231-256): X, X'', Y, Y'' per sample."""
        N = self.batch_size
        degs = self._grid_sizes(self.taylor_degree_range)
        tabs = []
        for k, n in enumerate((H, W)):
            pd = int(degs[k]) - 1                                     # polynomials_and_their_2nd_derivatives: poly_deg -= 1
            coeffs = 2 * self.rng.uniform(size=(N, pd)) - 1
            if self.homogeneous_bc:
                roots = -self.rng.uniform(size=(N, pd, max(pd - 1, 0)))
                roots = np.concatenate([np.zeros((N, pd, 1)), -np.ones((N, pd, 1)), roots], -1)
            else:
                roots = -self.rng.uniform(size=(N, pd, pd + 2))
            x = np.linspace(0.0, 1.0, n)
            P, D = np.zeros((N, n)), np.zeros((N, n))
            for b in range(N):
                for i in range(pd):
                    p, ddp = _poly_and_second_derivative(roots[b, i, :i + 2], x)
                    P[b] += coeffs[b, i] * p
                    D[b] += coeffs[b, i] * ddp / domain_sizes[b, k] ** 2
            tabs.append((P, D))
        return tabs

    def _draw_series(self):
        """The host draws every analytic generator starts a batch with, in this order: mode counts per sample, the grid shape and spacings, the
        series coefficients (zero beyond a sample's own mode counts).  -> ncoef (N,2), H, W, dx (N,2), domain_sizes (N,2), coef (N,ka,kb)."""
        ncoef = self._draw_mode_counts()                                                                  # (N,2)
        shape, dx = self._shape_and_spacings()
        H, W = int(shape[0]), int(shape[1])
        coef = self._draw_coefficients(ncoef)
        domain_sizes = dx * np.array([H, W], dtype=np.float64)[None]     # L = dx * n (reverse.py:203), not dx*(n-1)
        return ncoef, H, W, dx, domain_sizes, coef

    def __getitem__(self, idx=0):
        N = self.batch_size
        ncoef, H, W, dx, domain_sizes, coef = self._draw_series()
        ka, kb = coef.shape[1:]
        A, B = np.arange(1, ka + 1, dtype=np.float64), np.arange(1, kb + 1, dtype=np.float64)
        adj = -((math.pi * A[None, :, None] / domain_sizes[:, 0, None, None]) ** 2 + (math.pi * B[None, None, :] / domain_sizes[:, 1, None, None]) ** 2)
        trig = 1 if self.neumann else 0
        if not self.neumann and not self.homogeneous_bc:
            cosc = np.zeros((N, ka, kb))
            for b in range(N):
                cosc[b, :ncoef[b, 0], :ncoef[b, 1]] = 2 * self.rng.uniform(size=(ncoef[b, 0], ncoef[b, 1])) - 1
        soln = K.series_synthesis(self._dev(coef), H, W, trig)
        rhs = K.series_synthesis(self._dev(coef * adj), H, W, trig)
        if not self.neumann and not self.homogeneous_bc:
            K.series_synthesis(self._dev(cosc), H, W, 1, out=soln, accumulate=True)
            K.series_synthesis(self._dev(cosc * adj), H, W, 1, out=rhs, accumulate=True)
        if not self.neumann and self.taylor_degree_range is not None:
            (X, Xdd), (Y, Ydd) = self._taylor_tables(H, W, domain_sizes)
            soln_t = K.separable_sum(self._dev(X[:, None]), self._dev(Y[:, None]))
            rhs_t = K.separable_sum(self._dev(np.stack([Xdd, X], 1)), self._dev(np.stack([Y, Ydd], 1)))
            s = K.max_abs_per_sample(rhs) / K.max_abs_per_sample(rhs_t)      # reverse.py:299-306
            K.scale_samples(rhs_t, s)
            K.scale_samples(soln_t, s)
            ops.axpby(1.0, rhs_t.view(N, H, W, 1), 1.0, rhs.view(N, H, W, 1))
            ops.axpby(1.0, soln_t.view(N, H, W, 1), 1.0, soln.view(N, H, W, 1))
        return self._normalize_and_pack(rhs, soln, dx, domain_sizes)

    def _normalize_and_pack(self, rhs, soln, dx, domain_sizes):
        """rhs, soln (N,H,W) -> the normalised batch ([rhs, (boundaries...), dx], soln)."""
        N, H, W = rhs.shape
        nz = self.normalizations
        if nz['rhs_max_magnitude'] is not False:                             # reverse.py:287-290
            f = K.set_max_magnitude(rhs, torch.full((N,), float(nz['rhs_max_magnitude']), device=self.device))
            K.scale_samples(soln, f)
        if nz['soln_max_magnitude'] is not False:
            K.set_max_magnitude(soln, torch.ones((N,), device=self.device))
        if nz['max_domain_size_squared']:
            K.scale_samples(soln, self._dev(1.0 / domain_sizes.max(1) ** 2))
        rhs, soln = rhs.view(N, 1, H, W), soln.view(N, 1, H, W)
        problem = []
        if self.return_rhses:
            problem.append(rhs)
        if self.return_boundaries:
            problem += [soln[:, :, 0, :], soln[:, :, -1, :], soln[:, :, :, 0], soln[:, :, :, -1]]      # _boundary_slices order (reverse.py:141-146)
        if self.return_dx:
            problem.append(self._dev(dx[:, :1] if self.uniform_grid_spacing else dx))
        return problem, soln


class reverse_poisson_dataset_generator_homogeneous_neumann(reverse_poisson_dataset_generator):
    """Cosine-only series: zero normal derivative on every edge, zero-mean RHS (dataset/generators/reverse_neumann.py:9-66)."""

    def __init__(self, batch_size, batches_per_epoch, random_output_shape_range, fourier_coeff_grid_size_range, grid_spacings_range=None, ndims=None,
                 return_rhses=True, return_dx=True, normalizations=None, uniform_grid_spacing=False, seed=0, device=None, shard=None):
        super().__init__(batch_size, batches_per_epoch, random_output_shape_range, fourier_coeff_grid_size_range, None, grid_spacings_range, ndims,
                         homogeneous_bc=False, return_rhses=return_rhses, return_boundaries=False, return_dx=return_dx, normalizations=normalizations,
                         uniform_grid_spacing=uniform_grid_spacing, seed=seed, device=device, shard=shard)
        self.neumann = True


def _axis_basis(neumann_lo, neumann_hi):
    """The series_pair_synthesis basis of an axis from the types of its two ends and the offset of its frequencies (omega = A - offset, A = 1..k):
    (D,D) sin(A t), (N,N) cos(A t), (D,N) sin((A-1/2) t), (N,D) cos((A-1/2) t) - the eigenfunctions of -d2/dt2 on [0, pi] with u = 0 at a
    Dirichlet end and u' = 0 at a Neumann end."""
    mixed = bool(neumann_lo) != bool(neumann_hi)
    return (1 if neumann_lo else 0) | (2 if mixed else 0), (0.5 if mixed else 0.0)


class reverse_poisson_dataset_generator_mixed(reverse_poisson_dataset_generator):
    """Analytic pairs with a boundary type per edge and homogeneous data on every edge (u = 0 on a Dirichlet edge, du/dn = 0 on a Neumann one):
    the tensor product of the per-axis eigenfunction families of _axis_basis, (left, right) choosing the family along axis -2 and (bottom, top)
    the one along axis -1.  All-Dirichlet / all-Neumann flags give the sine / cosine series of the two generators above; the reference has no
    mixed analytic generator.  The host draws are the parent's (same seed, same coefficients); soln and rhs come from ONE launch
    (K.series_pair_synthesis) with the eigenvalues lam = -(pi omega / L)^2, L = dx * n as in the parent (reverse.py:203)."""

    def __init__(self, batch_size, batches_per_epoch, random_output_shape_range, fourier_coeff_grid_size_range, boundary_types, grid_spacings_range=None,
                 ndims=None, return_rhses=True, return_dx=True, normalizations=None, uniform_grid_spacing=False, seed=0, device=None, shard=None):
        super().__init__(batch_size, batches_per_epoch, random_output_shape_range, fourier_coeff_grid_size_range, None, grid_spacings_range, ndims,
                         homogeneous_bc=True, return_rhses=return_rhses, return_boundaries=False, return_dx=return_dx, normalizations=normalizations,
                         uniform_grid_spacing=uniform_grid_spacing, seed=seed, device=device, shard=shard)
        self.neumann_flags = _neumann_flags(boundary_types)              # (left, right, bottom, top)

    def __getitem__(self, idx=0):
        _, H, W, dx, domain_sizes, coef = self._draw_series()
        nl, nr, nb, nt = self.neumann_flags
        lams, bases = [], []
        for axis, (lo, hi) in enumerate(((nl, nr), (nb, nt))):
            basis, offset = _axis_basis(lo, hi)
            omega = np.arange(1, coef.shape[1 + axis] + 1, dtype=np.float64) - offset
            lams.append(-(math.pi * omega[None, :] / domain_sizes[:, axis, None]) ** 2)
            bases.append(basis)
        soln, rhs = K.series_pair_synthesis(self._dev(coef), self._dev(lams[0]), self._dev(lams[1]), H, W, bases[0], bases[1])
        return self._normalize_and_pack(rhs, soln, dx, domain_sizes)


# ----------------------------------------------------------------------------- numerical (FD) generator
class numerical_dataset_generator(_generator):
    """Random smooth RHS / Dirichlet BCs (bicubic up-sampling of random control points) -> 5-point FD solve on the GPU (DST-I).
    Output order with return_keras_style: [rhs, left, top, right, bottom, dx] (dataset/generators/numerical.py:204-216)."""

    def __init__(self, batch_size=1, batches_per_epoch=1, randomize_rhs_smoothness=False, rhs_random_smoothness_range=(5, 20),
                 randomize_boundary_smoothness=False, boundary_random_smoothness_range=None, randomize_rhs_max_magnitude=False,
                 rhs_random_max_magnitude=1.0, randomize_boundary_max_magnitudes=False, boundary_random_max_magnitudes=None,
                 return_keras_style=True, exclude_zero_boundaries=False, seed=0, device=None, shard=None, **numerical_dataset_arguments):
        self.batch_size, self.batches_per_epoch = int(batch_size), int(batches_per_epoch)
        self.randomize_rhs_smoothness, self.rhs_random_smoothness_range = randomize_rhs_smoothness, rhs_random_smoothness_range
        self.randomize_boundary_smoothness = randomize_boundary_smoothness
        self.boundary_random_smoothness_range = boundary_random_smoothness_range or {k: [5, 20] for k in _BOUNDARY_KEYS}
        self.randomize_rhs_max_magnitude, self.rhs_random_max_magnitude = randomize_rhs_max_magnitude, rhs_random_max_magnitude
        self.randomize_boundary_max_magnitudes = randomize_boundary_max_magnitudes
        self.boundary_random_max_magnitudes = boundary_random_max_magnitudes or {k: 1.0 for k in _BOUNDARY_KEYS}
        self.return_keras_style, self.exclude_zero_boundaries = return_keras_style, exclude_zero_boundaries
        self.nda = dict(numerical_dataset_arguments)
        self.nda.pop('normalizations', None)
        self.rng, self.shape_rng, self.shard = _streams(seed, shard)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())

    def _edge(self, ctrl, length, max_magnitude):
        """One edge array (N, length): the smooth function through the already drawn control values ctrl (N, k), or zeros when ctrl is None."""
        if ctrl is None:
            return torch.zeros((self.batch_size, length), dtype=torch.float32, device=self.device)
        return self._smooth_field(ctrl[:, None, :], (1, length), max_magnitude).view(self.batch_size, length)

    def numerical_dataset(self, output_shape='random', dx='random', boundaries='random', rhses='random', rhs_smoothness=None, boundary_smoothness=None,
                          rhs_max_magnitude=1.0, boundary_max_magnitude=None, nonzero_boundaries=_BOUNDARY_KEYS, solver_method='multigrid',
                          return_rhs=True, return_boundaries=False, return_dx=False, return_shape=False, random_output_shape_range=((64, 85), (64, 85)),
                          random_dx_range=(0.005, 0.05), normalize_by_domain_size=False, uniformly_distributed_aspect_ratios=True, boundary_types=None):
        """numerical_dataset (dataset/generators/numerical.py:74-150).  solver_method 'multigrid' / 'multigrid_gpu' / 'cholesky' all map
        to the DST-I direct solve of the same 5-point system.

        boundary_types (extension): dict edge -> 'dirichlet' | 'neumann' (default all Dirichlet).  A Neumann
        edge's random smooth boundary function is its normal derivative du/dn; the discrete mixed-BC system is solved directly
        (mixed_bc_poisson_solve) - a true mixed Dirichlet/Neumann ground truth for BASELINE configs[2]."""
        N, rng, srng = self.batch_size, self.rng, self.shape_rng
        rank, world = self.shard
        boundary_max_magnitude = boundary_max_magnitude or {k: 1.0 for k in _BOUNDARY_KEYS}
        if isinstance(output_shape, str) and output_shape == 'random':       # the grid shape comes from the stream all ranks share (see _streams)
            if uniformly_distributed_aspect_ratios:
                ar = generate_uniformly_distributed_aspect_ratios(random_output_shape_range, None, 1, srng)
                shape, dxg = generate_output_shapes_and_grid_spacings_from_aspect_ratios(ar, random_output_shape_range, [list(random_dx_range)], constant_dx=True,
                                                                                         samples=N * world, rng=srng)
                output_shape = [int(s) for s in shape]
                if isinstance(dx, str) and dx == 'random':
                    dx = dxg[rank * N:(rank + 1) * N, :1]
            else:
                output_shape = [int(srng.integers(r[0], r[1])) for r in random_output_shape_range]
        if isinstance(dx, str) and dx == 'random':
            dx = rng.uniform(size=(N, 1)) * (random_dx_range[1] - random_dx_range[0]) + random_dx_range[0]
        elif isinstance(dx, float):
            dx = np.ones((N, 1)) * dx
        dx = np.asarray(dx, dtype=np.float64).reshape(N, 1)
        H, W = output_shape
        if isinstance(rhses, str) and rhses == 'random':
            nc = rhs_smoothness
            if nc is None:
                nc = [int(rng.integers(5, int(n // 1.5))) for n in (H, W)]
            elif isinstance(nc, int):
                nc = [nc, nc]
            rhs = self._smooth_field(2 * rng.uniform(size=(N, nc[0], nc[1])) - 1, (H, W), rhs_max_magnitude)
        elif isinstance(rhses, str) and rhses == 'zero':
            rhs = torch.zeros((N, H, W), dtype=torch.float32, device=self.device)
        else:
            rhs = self._dev(np.asarray(rhses)).view(N, H, W)
        lengths = {'left': W, 'right': W, 'top': H, 'bottom': H}          # numerical.py:54
        if isinstance(boundaries, str):
            nonzero = list(nonzero_boundaries) if boundaries == 'random' else []
            sm = boundary_smoothness
            if isinstance(sm, int):
                sm = {k: sm for k in _BOUNDARY_KEYS}
            elif sm is None:
                sm = {k: int(rng.integers(5, int(lengths[k] // 1.5))) for k in _BOUNDARY_KEYS}
            bc = {k: self._edge(2 * rng.uniform(size=(N, sm[k])) - 1 if k in nonzero else None, lengths[k], boundary_max_magnitude[k]) for k in _BOUNDARY_KEYS}
        else:
            bc = {k: self._dev(np.asarray(boundaries[k])).view(N, lengths[k]) for k in _BOUNDARY_KEYS}
        if boundary_types is not None and any(str(v).lower() == 'neumann' for v in boundary_types.values()):
            soln = K.fd_poisson_mixed(rhs, bc['left'], bc['right'], bc['bottom'], bc['top'], self._dev(dx[:, 0]), _neumann_flags(boundary_types))
        else:
            soln = K.fd_poisson_dst(rhs, bc['left'], bc['right'], bc['bottom'], bc['top'], self._dev(dx[:, 0]))
        if normalize_by_domain_size:
            K.scale_samples(soln, self._dev(10.0 / (dx[:, 0] ** 2 * (H - 1) * (W - 1))))
        inp = []
        if return_rhs:
            inp.append(rhs.view(N, 1, H, W))
        if return_boundaries:
            inp.append({k: v.view(N, 1, -1) for k, v in bc.items()})
        if return_dx:
            inp.append(self._dev(dx))
        if return_shape:
            inp.append(torch.tensor([N, 1, H, W], dtype=torch.int32))
        soln = soln.view(N, 1, H, W)
        return (inp, soln) if inp else soln

    def __getitem__(self, idx=0):
        nda, rng = dict(self.nda), self.rng
        if self.randomize_rhs_smoothness:
            nda['rhs_smoothness'] = int(rng.integers(self.rhs_random_smoothness_range[0], self.rhs_random_smoothness_range[1]))
        if self.randomize_boundary_smoothness:
            nda['boundary_smoothness'] = {k: int(rng.integers(v[0], v[1])) for k, v in self.boundary_random_smoothness_range.items()}
        if self.randomize_rhs_max_magnitude:
            nda['rhs_max_magnitude'] = rng.uniform() * self.rhs_random_max_magnitude
        if self.randomize_boundary_max_magnitudes:
            nda['boundary_max_magnitude'] = {k: rng.uniform() * v for k, v in self.boundary_random_max_magnitudes.items()}
        inp, out = self.numerical_dataset(**nda)
        if self.return_keras_style and nda.get('return_boundaries', False):
            loc = 1 if nda.get('return_rhs', True) else 0
            b = inp.pop(loc)
            keys = _BOUNDARY_KEYS if (not self.exclude_zero_boundaries or 'nonzero_boundaries' not in nda) else nda['nonzero_boundaries']
            inp[loc:loc] = [b[k] for k in keys]
        return inp, out


# ----------------------------------------------------------------------------- solver entry points (dataset/solvers)
def _f32(a, device):
    return (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(device=device, dtype=torch.float32)


def _solver_args(rhses, boundaries, dx, device=None):
    """What every solver entry point accepts -> (rhs (N,H,W), edges dict, dx (N,), device), all fp32, contiguous and on `device` (default: the
    current CUDA device).  rhses (N,1,H,W) or (N,H,W), numpy or torch; boundaries: 'left'/'right' (N,W) and 'bottom'/'top' (N,H), extra
    singleton dims allowed, a batch of 1 is broadcast to N; dx: one number, (N,), (N,1) or (N,2) - the first column."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    r = _f32(rhses, dev)
    if r.dim() == 4:
        r = r[:, 0]
    N, H, W = r.shape
    b = {k: _f32(boundaries[k], dev).reshape(-1, W if k in ('left', 'right') else H).expand(N, -1).contiguous() for k in _BOUNDARY_KEYS}
    d = _f32(dx, dev).reshape(-1)
    d = d.expand(N).contiguous() if d.numel() == 1 else d.reshape(N, -1)[:, 0].contiguous()
    return r.contiguous(), b, d, dev


def multigrid_poisson_solve(rhses, boundaries, dx, dy=None, system_matrix=None, tol=1e-10, solver_init_parameters=None, solver_run_parameters=None,
                            use_pyamgx=False, initial_guesses=None, device=None):
    """Drop-in for dataset/solvers/multigrid.py:98-150: solves pyamg.gallery.poisson((H-2, W-2)) u = poisson_RHS(rhses, boundaries, dx)
    and writes the Dirichlet values - by the direct DST-I diagonalisation on the GPU instead of Ruge-Stuben V-cycles / AMGX
    (tol, solver parameters and initial guesses are accepted and irrelevant for a direct solve; like the reference only `dx` is used).
    rhses (N,1,H,W) or (N,H,W); boundaries: dict with 'left'/'right' (N,W) and 'bottom'/'top' (N,H) (extra singleton dims allowed)."""
    r, b, d, _ = _solver_args(rhses, boundaries, dx, device)
    return K.fd_poisson_dst(r, b['left'], b['right'], b['bottom'], b['top'], d).unsqueeze(1)


def cholesky_poisson_solve(rhses, boundaries, h, system_matrix=None, system_matrix_is_decomposed=False, device=None):
    """dataset/solvers/cholesky.py:122-186 (dense Cholesky of the same 5-point matrix): same system, same direct DST-I solve."""
    return multigrid_poisson_solve(rhses, boundaries, h, device=device)


def mixed_bc_poisson_solve(rhses, boundaries, dx, boundary_types, device=None):
    """5-point FD Poisson solve with per-edge Dirichlet / Neumann conditions on the reference's vertex-centred grid (same edge naming and
    array shapes as multigrid_poisson_solve).  The reference has no such solver in its dataset path - its only Neumann data are analytic
    cosine series (dataset/generators/reverse_neumann.py) - but its Navier-Stokes projection step solves exactly this system
    (Navier_Stokes_2D/solvers.py:225-335, zero-integral constraint for the singular all-Neumann case, :258-259).
    boundary_types: dict edge -> 'dirichlet' | 'neumann'; a Neumann edge's array holds du/dn along the outward normal."""
    r, b, d, _ = _solver_args(rhses, boundaries, dx, device)
    return K.fd_poisson_mixed(r, b['left'], b['right'], b['bottom'], b['top'], d, _neumann_flags(boundary_types)).unsqueeze(1)


# ----------------------------------------------------------------------------- variable-density problem (dataset/generators/variable_density)
def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _per_sample_spacing(v, N):
    """One spacing, (N,), (N,1) or (N,2) -> (N,): the first column, as multigrid_poisson_solve reads it."""
    return np.full((N,), float(v.reshape(-1)[0])) if v.size == 1 else v.reshape(N, -1)[:, 0]


def _lead_shape(a, name, dims):
    s = tuple(a.shape)
    if len(s) == dims + 1 and s[1] == 1:
        s = s[:1] + s[2:]
    if len(s) != dims:
        raise ValueError('%s must have %d dimensions (a singleton channel axis is allowed), got shape %r' % (name, dims, tuple(a.shape)))
    return s


VARIABLE_DENSITY_PRECONDITIONERS = ('dst', 'scaled')
VARIABLE_DENSITY_PROFILES = ('abs', 'smooth')


def _reaction_on_host(reaction, rs, neumann, preconditioner):
    """The refusals of variable_density_poisson_solve's `reaction` that need no device; -> True when it is one number per sample (or one number)."""
    N, H, W = rs
    if preconditioner == 'scaled':
        raise ValueError("preconditioner='scaled' has no reaction variant: use 'dst' with reaction")
    shape = tuple(reaction.shape) if hasattr(reaction, 'shape') else np.shape(reaction)
    per_sample = int(np.prod(shape, dtype=np.int64)) in (1, N) and len(shape) <= 4 and all(d == 1 for d in shape[1:])
    if not per_sample and _lead_shape(reaction, 'reaction', 3) != rs:
        raise ValueError('reaction %r must match rhses %r, or hold one number per sample' % (shape, rs))
    if not (isinstance(reaction, torch.Tensor) and reaction.is_cuda):            # a device tensor is checked by the setup launch
        c = _host_array(reaction).astype(np.float64)
        (i0, i1), (j0, j1) = K.varcoef_unknowns(H, W, neumann)
        c = np.broadcast_to(c.reshape(-1, 1, 1), (N, 1, 1)) if per_sample else c.reshape(N, H, W)[:, i0:i1 + 1, j0:j1 + 1]
        if not np.all(np.isfinite(c) & (c >= 0)):
            raise ValueError('reaction must be non-negative and finite on every unknown')
        zero = np.flatnonzero(~(c.reshape(N, -1) > 0).any(axis=1))
        if all(neumann) and zero.size:
            raise ValueError('all four edges Neumann and a reaction that is zero on every unknown of sample(s) %r: that system is singular - solve such a '
                             'sample without the reaction keyword' % (zero.tolist(),))
    return per_sample


def variable_density_poisson_solve(rho, rhses, boundaries, dx, dy=None, tol=1e-10, max_iterations=500, initial_guesses=None, check_every=8,
                                   return_info=False, device=None, check_start=False, boundary_types=None, preconditioner='dst', reaction=None):
    """Solves div((1/rho) grad u) = f with Dirichlet data on the four edges, on the vertex-centred grid of multigrid_poisson_solve (same shapes
    and edge names: rhses (N,1,H,W) or (N,H,W); boundaries: dict with 'left'/'right' (N,W) and 'bottom'/'top' (N,H); dx one spacing per sample).
    rho (N,H,W) or (N,1,H,W) is given on every node, boundary nodes included, and must be positive.

    Discretisation: the conservative (flux) form with the face coefficients beta = 2 / (rho_a + rho_b) of the two nodes a face separates - the
    first matrix of the reference's dataset/generators/variable_density, c = 2 / (dx^2 (rho_c + rho_neighbour)).  With A = -L this is a symmetric
    positive definite system A u = b on the (H-2) x (W-2) interior nodes; rho = c everywhere gives the system of multigrid_poisson_solve with
    f replaced by c f.  The reference's third matrix - the non-conservative form (1/rho) lap u + grad(1/rho).grad u with identity rows for the
    boundary nodes - is nonsymmetric and is NOT reproduced.  Only dy = dx is supported: a dy that differs from dx raises NotImplementedError.

    Solver: conjugate gradients in fp64 on the GPU, preconditioned by the constant-coefficient DST solve (condition number at most
    max(beta) / min(beta), whatever the grid size).  A sample stops changing once ||r|| <= tol ||b||; the host looks at the convergence flags
    every `check_every` iterations, so max_iterations is rounded up to a multiple of check_every.  initial_guesses: optional (N,H,W) or
    (N,1,H,W) start values (read in fp64; only the interior is used).  A sample that has not converged when the iterations run out raises a
    RuntimeWarning and is reported as converged = False.  check_start=True also looks at the flags before the first iteration: a start that
    already meets the tolerance then reports 0 iterations (by default the first look comes after check_every iterations); the solution is the
    same, bit for bit.

    boundary_types: dict edge -> 'dirichlet' | 'neumann' as mixed_bc_poisson_solve takes it (a missing edge is Dirichlet); None or all Dirichlet is
    the solve described above, untouched.  A Neumann edge's array holds g = du/dn along the outward normal, its nodes are unknowns (rho and f are
    read there too) and a Dirichlet edge wins a corner; a Dirichlet node has the value the edge arrays give it, rows 0 / H-1 first.  With A = -L:
      rows   (A u)_c = sum_k beta_k (u_c - u_k) / dx^2 over the four directions; a Neumann edge node has no outward neighbour and the inward face
             of that direction counts twice, 2 beta_in (u_c - u_in) (both directions at a Neumann/Neumann corner); faces along the edge are ordinary.
      b      -f_c, plus beta_k / dx^2 times each Dirichlet neighbour's value, plus 2 g / (rho_c dx) for each Neumann edge that contains the node:
             1 / rho_c is the coefficient on the boundary face of the node's half cell.  (The mirrored ghost node's 2 beta_in g / dx is first order;
             this form is second order.)
      w      = w_i w_j with 1/2 on a Neumann edge's row / column, else 1: W A is symmetric - positive definite with a Dirichlet edge - and the
             solver is conjugate gradients in the W inner product, preconditioned by the constant-coefficient solve of the same edge types
             (mixed_bc_poisson_solve's): a sample stops at sum w r^2 <= tol^2 sum w b^2, and the condition number bound above carries over.
             rho = c everywhere gives mixed_bc_poisson_solve's system with f replaced by c f.
      all four Neumann: W A has the constants as null space.  b is replaced by b - (sum w b) / (sum w), the compatibility projection, and the
             returned solution has zero trapezoidal integral (mixed_bc_poisson_solve's convention), whatever mean the initial guess has.  info's
             `compatibility_defect` = |sum w b| / sqrt(sum w * sum w b^2) in [0, 1] tells how incompatible the data were, and `rhs_shift` the
             constant the projection added to f: the solution satisfies the discrete equation of f + rhs_shift.

    preconditioner: 'dst' (default) is the constant-coefficient solve M^-1 described above.  'scaled' is Concus and Golub's diagonal scaling of
    it, z = s o M^-1 (s o r) with s = d^-1/2 and d the mean of the node's four face coefficients (diag(A) / diag(M); on a Neumann edge the inward
    face twice): for a SMOOTH rho the iteration count then follows the derivatives of log rho and no longer max rho / min rho - 13 to 25 iterations
    against 41 to 159 at ratio 1000 in the fp64 twin - at the same launches per iteration (2 to 4 % more time each).  For a rho with kinks or jumps
    (the generator's default 'abs' profile has kinks) it gains nothing and takes MORE iterations than 'dst' on fine grids (3 to 4 times as many at
    512^2 and ratio 100 to 1000): opt-in, DESIGN.md section 22 has the counts.  Works with every
    boundary_types and with initial_guesses; the same system, tolerance and returned info.  Any other value raises ValueError.

    reaction: c >= 0 in div((1/rho) grad u) - c u = f - the implicit diffusion or viscous step (rho / dt) u - div(mu grad u) = g
    and any backward-Euler step of u_t = div(k grad u) have this form.  fp32, (N,H,W) or (N,1,H,W) on every node, or one number per sample ((N,),
    (N,1), ..) that is broadcast; read on the unknowns only.  On the unknowns (A + C) u = b with C = diag(c) and the A, b and w above; W (A + C) is
    symmetric and positive definite once an edge is Dirichlet or c > 0 somewhere.  The preconditioner becomes the constant-coefficient solve of
    bbar M + cbar I - bbar and cbar the weighted means of 1/rho and of c over the unknowns, M with its 1/dx^2 - and the condition number is at most
    max(beta/bbar, c/cbar) / min(beta/bbar, c/cbar) at any grid size.  That bound is weak when c dominates the operator's diagonal AND varies as
    much as 1/rho does: with c = 1e3 s / (rho dx^2), s in [0.5, 1.5], the device needs 56 to 64 iterations at density ratio 10 (40 without c) but
    472 to more than 504 at ratio 1000 (264 to 288 without c) on 512^2 grids - raise max_iterations there.  With all four edges Neumann and c > 0 somewhere the system is nonsingular:
    nothing is projected, no mean is removed, `compatibility_defect` and `rhs_shift` are zeros.  ValueError: a c that is negative or not finite on
    an unknown (a host array: before any device work; a device tensor: straight after the setup launch, a NaN counting as -inf), a shape that
    matches neither form, preconditioner='scaled' together with reaction, and - all four edges Neumann - a sample whose c is zero on every unknown
    (singular: solve it without the keyword).  None (default): the solve above, the same calls and the same bits.

    Returns soln (N,1,H,W) fp32; with return_info also a dict of per-sample numpy arrays `iterations` (a multiple of check_every), `converged`
    and `relative_residual` (||r|| / ||b|| of the recurrence), and with a Neumann edge `compatibility_defect` and `rhs_shift` (zeros unless all four
    edges are Neumann)."""
    import warnings
    # everything that can be refused without a device is refused first
    neumann = _neumann_flags(boundary_types) if boundary_types is not None else (False,) * 4
    if preconditioner not in VARIABLE_DENSITY_PRECONDITIONERS:
        raise ValueError('preconditioner must be one of %r, got %r' % (VARIABLE_DENSITY_PRECONDITIONERS, preconditioner))
    rs = _lead_shape(rhses, 'rhses', 3)
    if _lead_shape(rho, 'rho', 3) != rs:
        raise ValueError('rho %r and rhses %r must have the same (N,H,W)' % (tuple(rho.shape), tuple(rhses.shape)))
    N, H, W = rs
    if H < 3 or W < 3:
        raise ValueError('the grid needs at least 3 points per axis, got %d x %d' % (H, W))
    two_columns = len(tuple(np.shape(dx))) == 2 and np.shape(dx)[1] == 2           # (N,2): dx and dy side by side, as the generators hand them out
    if dy is not None or two_columns:
        hx = _host_array(dx).astype(np.float64)
        hy = hx[:, 1] if dy is None else _host_array(dy).astype(np.float64)
        if not np.array_equal(_per_sample_spacing(hx, N), _per_sample_spacing(hy, N)):
            raise NotImplementedError('variable_density_poisson_solve: anisotropic spacing (dy != dx) is not supported')
    if not (float(tol) > 0.0):
        raise ValueError('tol must be positive')
    if int(max_iterations) < 1 or int(check_every) < 1:
        raise ValueError('max_iterations and check_every must be at least 1')
    missing = [k for k in _BOUNDARY_KEYS if k not in boundaries]
    if missing:
        raise ValueError('boundaries lacks %r' % (missing,))
    if initial_guesses is not None and _lead_shape(initial_guesses, 'initial_guesses', 3) != rs:
        raise ValueError('initial_guesses %r must match rhses %r' % (tuple(initial_guesses.shape), tuple(rhses.shape)))
    if not (isinstance(rho, torch.Tensor) and rho.is_cuda) and not np.all(_host_array(rho) > 0):
        raise ValueError('rho must be positive everywhere')
    reaction_per_sample = _reaction_on_host(reaction, rs, neumann, preconditioner) if reaction is not None else False
    r, b, d, dev = _solver_args(rhses, boundaries, dx, device)
    dens = _f32(rho, dev).reshape(N, H, W).contiguous()
    x0 = None
    if initial_guesses is not None:
        g = initial_guesses if isinstance(initial_guesses, torch.Tensor) else torch.as_tensor(np.asarray(initial_guesses))
        x0 = g.to(device=dev, dtype=torch.float64).reshape(N, H, W).contiguous()
    extra = {'scaled': True} if preconditioner == 'scaled' else {}              # ('dst': the call as it has always been)
    if reaction is not None:                                                    # (None: the call as it has always been; never with 'scaled')
        c = _f32(reaction, dev)
        extra = {'reaction': (c.reshape(-1, 1, 1).expand(N, H, W) if reaction_per_sample else c.reshape(N, H, W)).contiguous()}
    soln, info = K.varcoef_pcg_solve(dens, r, b['left'], b['right'], b['bottom'], b['top'], d, tol=float(tol), max_iterations=int(max_iterations), x0=x0,
                                     check_every=int(check_every), check_start=bool(check_start), neumann=neumann if any(neumann) else None, **extra)
    if not info['converged'].all():           # (a rho <= 0 or NaN on the device was refused inside, straight after the setup kernel's minimum)
        bad = np.flatnonzero(~info['converged'])
        warnings.warn('variable_density_poisson_solve: sample(s) %r not converged to tol = %g after %d iterations (relative residual %r)'
                      % (bad.tolist(), tol, int(info['iterations'].max()), info['relative_residual'][bad].tolist()), RuntimeWarning, stacklevel=2)
    soln = soln.view(N, 1, H, W)
    if return_info:
        keys = ('iterations', 'converged', 'relative_residual') + (('compatibility_defect', 'rhs_shift') if any(neumann) else ())
        return soln, {k: info[k] for k in keys}
    return soln


def compressible_poisson_solve(rho, rhses, boundaries, dx, dy=None, system_matrix=None, preconditioner='dst', reaction=None):
    """The reference's name and argument order (dataset/generators/variable_density: compressible_poisson_solve).  system_matrix is accepted and
    ignored: no matrix is assembled.  preconditioner, reaction: variable_density_poisson_solve's."""
    return variable_density_poisson_solve(rho, rhses, boundaries, dx, dy=dy, preconditioner=preconditioner, reaction=reaction)


def _check_density_range(density_range):
    lo, hi = float(density_range[0]), float(density_range[1])
    if not 0.0 < lo <= hi:
        raise ValueError('density_range = (lo, hi) needs 0 < lo <= hi, got %r' % (density_range,))
    return lo, hi


def _check_density_profile(density_profile):
    if density_profile not in VARIABLE_DENSITY_PROFILES:
        raise ValueError('density_profile must be one of %r, got %r' % (VARIABLE_DENSITY_PROFILES, density_profile))


def _check_smoothness_ranges(**ranges):
    for name, rg in ranges.items():
        if not 2 <= int(rg[0]) <= int(rg[1]):
            raise ValueError('%s = (lo, hi) needs 2 <= lo <= hi control points, got %r' % (name, rg))


class variable_density_dataset_generator(numerical_dataset_generator):
    """Random smooth right-hand side F and density rho -> the variable-density solve: generate_dataset of the reference's
    dataset/generators/variable_density, which returns (soln, stack([F, rho], axis=1)).  Keras order here (return_keras_style):
    ([stack([rhs, rho], axis=1), dx], soln), with the four boundary arrays (left, top, right, bottom, each (N,1,len)) between the stack and dx
    when boundaries = 'random'; otherwise the reference's pair (soln, stack).  Homogeneous_Poisson_NN_Legacy(density_input=True) reads the
    two-channel input (boundaries = 'zero'; train.py --dataset_type variable_density).

    rho = lo + (hi - lo) |g| / max|g| with g a smooth random field (the bicubic up-sampling of random control points the numerical generator
    uses) and (lo, hi) = density_range: the reference takes 1e-7 + |g|, whose ratio max/min is unbounded; density_range bounds the condition
    number of the preconditioned system by hi / lo.  One grid shape per batch (output_shape, or drawn from random_output_shape_range), one
    spacing per sample from random_dx_range.

    boundary_types: dict edge -> 'dirichlet' | 'neumann' (variable_density_poisson_solve's; None: all Dirichlet).  A Neumann edge's array is its
    du/dn: zeros with boundaries = 'zero', the drawn smooth function with 'random' - the draws are the same whatever the types.  With all four
    edges Neumann the right-hand side returned is the one the solution satisfies: the drawn one plus the constant of the solver's compatibility
    projection (last_info['rhs_shift']).  Homogeneous_Poisson_NN_Legacy(density_input=True, boundary_types=...) trains on such batches (DESIGN.md
    section 20).

    density_profile: 'abs' (default) is the rho above, which has a kink wherever g changes sign.  'smooth' is rho = lo + (hi - lo) (g - min g) /
    (max g - min g) per sample (pcnn_varcoef_density_smooth): as smooth as g, minimum lo and maximum hi - the densities preconditioner = 'scaled'
    (variable_density_poisson_solve's, passed through; default 'dst') is for.  Neither changes the random draws.

    reaction_range: (lo, hi) with 0 <= lo <= hi draws one more smooth field c = lo + (hi - lo) |g| / max|g| (density_smoothness_range control
    points, the density kernel's map), solves div((1/rho) grad u) - c u = f with it (variable_density_poisson_solve's reaction) and yields it as a
    third channel, stack([rhs, rho, c], axis=1).  The field is drawn last, after the edges: the draws of every other field are those of
    reaction_range = None, which is the generator above, draw for draw.  Not with preconditioner = 'scaled'; with all four edges Neumann lo or hi
    must be positive enough that no sample's c vanishes (the solve refuses such a sample).  The model's density_input reads two channels: such
    batches are for solver studies, not yet for training."""

    def __init__(self, batch_size=1, batches_per_epoch=1, output_shape=None, random_output_shape_range=((64, 85), (64, 85)), density_range=(1.0, 10.0),
                 rhs_smoothness_range=(5, 20), density_smoothness_range=(5, 20), boundaries='zero', random_dx_range=(0.005, 0.05), rhs_max_magnitude=1.0,
                 boundary_max_magnitude=1.0, tol=1e-10, max_iterations=500, seed=0, device=None, return_keras_style=True, shard=None, boundary_types=None,
                 preconditioner='dst', density_profile='abs', reaction_range=None):
        super().__init__(batch_size=batch_size, batches_per_epoch=batches_per_epoch, return_keras_style=return_keras_style, seed=seed, device=device,
                         shard=shard)
        if reaction_range is not None:
            if len(reaction_range) != 2 or not 0.0 <= float(reaction_range[0]) <= float(reaction_range[1]) < np.inf:
                raise ValueError('reaction_range = (lo, hi) needs 0 <= lo <= hi, got %r' % (reaction_range,))
            if preconditioner == 'scaled':
                raise ValueError("preconditioner='scaled' has no reaction variant: use 'dst' with reaction_range")
            reaction_range = (float(reaction_range[0]), float(reaction_range[1]))
        self.reaction_range = reaction_range
        self.boundary_types = boundary_types
        self.neumann_flags = _neumann_flags(boundary_types) if boundary_types is not None else (False,) * 4      # (left, right, bottom, top)
        lo, hi = _check_density_range(density_range)
        if boundaries not in ('zero', 'random'):
            raise ValueError("boundaries must be 'zero' or 'random'")
        if preconditioner not in VARIABLE_DENSITY_PRECONDITIONERS:
            raise ValueError('preconditioner must be one of %r, got %r' % (VARIABLE_DENSITY_PRECONDITIONERS, preconditioner))
        _check_density_profile(density_profile)
        self.preconditioner, self.density_profile = preconditioner, density_profile
        _check_smoothness_ranges(rhs_smoothness_range=rhs_smoothness_range, density_smoothness_range=density_smoothness_range)
        self.output_shape = None if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        self.random_output_shape_range = np.asarray(random_output_shape_range, dtype=np.int64).reshape(2, 2)
        self.density_range = (lo, hi)
        self.rhs_smoothness_range, self.density_smoothness_range = tuple(rhs_smoothness_range), tuple(density_smoothness_range)
        self.boundaries, self.random_dx_range = boundaries, (float(random_dx_range[0]), float(random_dx_range[1]))
        self.rhs_max_magnitude, self.boundary_max_magnitude = float(rhs_max_magnitude), float(boundary_max_magnitude)
        self.tol, self.max_iterations = float(tol), int(max_iterations)
        self.last_info = None          # iterations / converged / relative_residual of the latest batch

    def __getitem__(self, idx=0):
        N, rng = self.batch_size, self.rng
        if self.output_shape is not None:
            H, W = self.output_shape
        else:
            H, W = [int(self.shape_rng.integers(r[0], r[1] + 1)) for r in self.random_output_shape_range]
        dx = rng.uniform(size=(N, 1)) * (self.random_dx_range[1] - self.random_dx_range[0]) + self.random_dx_range[0]
        ctrl_counts = lambda rg: [int(rng.integers(rg[0], rg[1] + 1)) for _ in range(2)]
        nf, nr = ctrl_counts(self.rhs_smoothness_range), ctrl_counts(self.density_smoothness_range)
        rhs = self._smooth_field(2 * rng.uniform(size=(N, nf[0], nf[1])) - 1, (H, W), self.rhs_max_magnitude)
        rho = self._density_field(2 * rng.uniform(size=(N, nr[0], nr[1])) - 1, (H, W))
        lengths = {'left': W, 'right': W, 'top': H, 'bottom': H}
        bc = {}
        for k in _BOUNDARY_KEYS:
            ctrl = None
            if self.boundaries == 'random':                                # count, then values, edge by edge
                nb = int(rng.integers(self.rhs_smoothness_range[0], self.rhs_smoothness_range[1] + 1))
                ctrl = 2 * rng.uniform(size=(N, nb)) - 1
            bc[k] = self._edge(ctrl, lengths[k], self.boundary_max_magnitude)
        d = self._dev(dx)
        extra = {}
        if self.reaction_range is not None:                                # drawn last: the streams of the fields above do not move
            nc = ctrl_counts(self.density_smoothness_range)
            extra['reaction'] = K.varcoef_reaction_field(self._smooth_field(2 * rng.uniform(size=(N, nc[0], nc[1])) - 1, (H, W), 1.0), *self.reaction_range)
        soln, self.last_info = variable_density_poisson_solve(rho, rhs, bc, d, tol=self.tol, max_iterations=self.max_iterations, return_info=True,
                                                              device=self.device, boundary_types=self.boundary_types, preconditioner=self.preconditioner,
                                                              **extra)
        if all(self.neumann_flags) and not extra:                          # the equation (rhs, soln) satisfies: the solver projected its b
            rhs = rhs + torch.as_tensor(self.last_info['rhs_shift'], dtype=torch.float32, device=rhs.device).view(N, 1, 1)
        frho = torch.stack([rhs, rho] + list(extra.values()), dim=1)
        if not self.return_keras_style:
            return soln, frho
        inp = [frho]
        if self.boundaries == 'random':
            inp += [bc[k].view(N, 1, -1) for k in _BOUNDARY_KEYS]
        return inp + [d], soln


class reverse_variable_density_dataset_generator(_generator):
    """Solve-free pairs of the variable-density problem div((1/rho) grad u) = f: a random series u in the homogeneous
    eigenfunction families of the edge types (reverse_poisson_dataset_generator_mixed's: u = 0 on a Dirichlet edge, du/dn = 0 on a Neumann one), a
    random rho, and the DISCRETE right-hand side f = L_h(rho) u of the flux form the solver, the loss, the smoother and the metrics share - one
    launch (K.varcoef_series_pair: u is synthesised and differenced in fp64, only soln and rhs are rounded), whatever the density ratio.  The target
    is what variable_density_poisson_solve returns for that rhs and rho, to the fp32 rounding of the two fields.

    Yields variable_density_dataset_generator's structure for boundaries = 'zero': ([stack([rhs, rho], axis=1), dx], soln) with return_keras_style,
    else the reference's pair (soln, stack); Homogeneous_Poisson_NN_Legacy(density_input=True, boundary_types=...) trains on it (train.py
    --dataset_type variable_density_analytical).  The data differ in kind: here u is band limited (fourier_coeff_grid_size_range modes per axis,
    at most 16) and rhs inherits rho's kinks; the solver-made batches have independent smooth rhs and rho.

    Mode counts and coefficients are drawn as reverse_poisson_dataset_generator draws them, rho as variable_density_dataset_generator draws it
    (density_range, density_smoothness_range, density_profile), one grid shape per batch (output_shape, or drawn from random_output_shape_range)
    and one spacing per sample from random_dx_range.  The problem is linear in (u, f): each sample's rhs and soln are scaled by one factor so that
    max|rhs| = rhs_max_magnitude (None: as synthesised); rho is untouched.  boundary_types: dict edge -> 'dirichlet' | 'neumann' (None: all
    Dirichlet).  With all four edges Neumann the cosine modes A >= 1 have zero trapezoidal sum on the grid: soln has the zero weighted integral
    of the solver's convention and rhs is compatible by construction - no projection, no rhs_shift."""

    def __init__(self, batch_size=1, batches_per_epoch=1, fourier_coeff_grid_size_range=(1, 8), output_shape=None,
                 random_output_shape_range=((64, 85), (64, 85)), density_range=(1.0, 10.0), density_smoothness_range=(5, 20), density_profile='abs',
                 random_dx_range=(0.005, 0.05), boundary_types=None, rhs_max_magnitude=1.0, seed=0, device=None, return_keras_style=True, shard=None):
        # everything that can be refused without a device is refused first
        self.batch_size, self.batches_per_epoch = int(batch_size), int(batches_per_epoch)
        self.boundary_types = boundary_types
        self.neumann_flags = _neumann_flags(boundary_types) if boundary_types is not None else (False,) * 4      # (left, right, bottom, top)
        self.density_range = _check_density_range(density_range)
        _check_density_profile(density_profile)
        self.density_profile = density_profile
        _check_smoothness_ranges(density_smoothness_range=density_smoothness_range)
        self.density_smoothness_range = tuple(density_smoothness_range)
        fr = np.asarray(fourier_coeff_grid_size_range, dtype=np.float64)
        fr = np.tile(fr[None], (2, 1)) if fr.ndim == 1 else fr
        if fr.shape != (2, 2) or not np.all((0 <= fr[:, 0]) & (fr[:, 0] <= fr[:, 1])):
            raise ValueError('fourier_coeff_grid_size_range = (lo, hi), or one such pair per axis, needs 0 <= lo <= hi, got %r' % (fourier_coeff_grid_size_range,))
        most = np.where(fr[:, 0] == fr[:, 1], np.floor(fr[:, 1] + 1), np.ceil(fr[:, 1] + 1) - 1)          # the largest count _grid_sizes can return
        if most.max() > ops.VARCOEF_SERIES_MAX_MODES:
            raise ValueError('fourier_coeff_grid_size_range %r allows %d modes along an axis: the series kernel takes at most %d'
                             % (fourier_coeff_grid_size_range, int(most.max()), ops.VARCOEF_SERIES_MAX_MODES))
        self.fourier_coeff_grid_size_range = fr
        if output_shape is not None and (len(output_shape) != 2 or min(int(s) for s in output_shape) < 3):
            raise ValueError('output_shape = (H, W) needs at least 3 points per axis, got %r' % (output_shape,))
        self.output_shape = None if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
        self.random_output_shape_range = np.asarray(random_output_shape_range, dtype=np.int64).reshape(2, 2)
        if output_shape is None and not np.all((3 <= self.random_output_shape_range[:, 0]) & (self.random_output_shape_range[:, 0] <= self.random_output_shape_range[:, 1])):
            raise ValueError('random_output_shape_range = ((lo, hi), (lo, hi)) needs 3 <= lo <= hi points per axis, got %r' % (random_output_shape_range,))
        self.random_dx_range = (float(random_dx_range[0]), float(random_dx_range[1]))
        if not 0.0 < self.random_dx_range[0] <= self.random_dx_range[1]:
            raise ValueError('random_dx_range = (lo, hi) needs 0 < lo <= hi, got %r' % (random_dx_range,))
        if rhs_max_magnitude is not None and not float(rhs_max_magnitude) > 0.0:
            raise ValueError('rhs_max_magnitude must be positive or None, got %r' % (rhs_max_magnitude,))
        self.rhs_max_magnitude = None if rhs_max_magnitude is None else float(rhs_max_magnitude)
        self.return_keras_style = return_keras_style
        self.rng, self.shape_rng, self.shard = _streams(seed, shard)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())

    def __getitem__(self, idx=0):
        N, rng = self.batch_size, self.rng
        if self.output_shape is not None:
            H, W = self.output_shape
        else:                                                              # the grid shape comes from the stream all ranks share (see _streams)
            H, W = [int(self.shape_rng.integers(r[0], r[1] + 1)) for r in self.random_output_shape_range]
        dx = rng.uniform(size=(N, 1)) * (self.random_dx_range[1] - self.random_dx_range[0]) + self.random_dx_range[0]
        coef = self._draw_coefficients(self._draw_mode_counts())
        nr = [int(rng.integers(self.density_smoothness_range[0], self.density_smoothness_range[1] + 1)) for _ in range(2)]
        rho = self._density_field(2 * rng.uniform(size=(N, nr[0], nr[1])) - 1, (H, W))
        d = self._dev(dx)
        soln, rhs = K.varcoef_series_pair(self._dev(coef), rho, d, self.neumann_flags)
        if self.rhs_max_magnitude is not None:                             # linear in (u, f): one factor per sample for both
            K.scale_samples(soln, K.set_max_magnitude(rhs, torch.full((N,), self.rhs_max_magnitude, device=self.device)))
        frho = torch.stack([rhs, rho], dim=1)
        soln = soln.view(N, 1, H, W)
        if not self.return_keras_style:
            return soln, frho
        return [frho, d], soln
