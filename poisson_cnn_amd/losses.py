"""loss_wrapper / integral_loss / linear_operator_loss on the libpcnn loss kernels.

Drop-in for poisson_CNN/losses/loss_wrapper.py:6-71 (same constructor kwargs: the "loss_parameters" section of
experiments/hpnn.json loads unchanged; `loss(y_true, y_pred, rhs, dx)`), plus `value_and_grad` used by the model's
train_step instead of a GradientTape.
"""
import numpy as np
import torch

from . import ops
from ctypes import c_float, c_int, c_int64


def get_fd_coefficients(stencil_positions, order):
    """dataset/utils/get_fd_coefficients.py:4-19."""
    from math import factorial
    pos = np.array(sorted(stencil_positions), dtype=np.float64)
    V = np.vander(pos, increasing=True).T
    rhs = np.zeros(len(pos))
    rhs[order] = factorial(order)
    return np.linalg.solve(V, rhs)


def build_fd_coefficients(stencil_size, orders, ndims=None):
    """dataset/utils/build_fd_coefficients.py:5-42."""
    if ndims is None:
        ndims = len(stencil_size)
    if isinstance(stencil_size, int):
        stencil_size = [stencil_size] * ndims
    if isinstance(orders, int):
        orders = [orders] * ndims
    ss = np.array(stencil_size, dtype=int)
    if len(ss) == 1:
        ss = np.repeat(ss, ndims)
    assert len(ss) == ndims and np.all(ss % 2 == 1), 'Stencil sizes must be all odd'
    coeff = np.zeros([ndims] + list(ss))
    for d in range(ndims):
        sl = [d] + list(ss // 2)
        sl[d + 1] = slice(0, ss[d])
        coeff[tuple(sl)] += get_fd_coefficients(list(range(-(ss[d] // 2), ss[d] // 2 + 1)), int(orders[d]))
    return coeff


class integral_loss:
    """losses/integral_loss.py:80-179.  The Gauss-Legendre integral of the multilinear interpolant of (y-t)^p is a fixed
    linear functional of the grid values, so it is applied as one (H,W) weight map G: L = sum(G * (y-t)^p) * vol / 2^d."""

    def __init__(self, n_quadpts, ndims=None, Lp_norm_power=2, data_format='channels_first', reduce_results=False):
        if ndims is None:
            ndims = len(n_quadpts)
        if ndims != 2 or data_format != 'channels_first':
            raise NotImplementedError('integral_loss: 2-D channels_first only')
        self.n_quadpts = [n_quadpts] * ndims if isinstance(n_quadpts, int) else list(n_quadpts)
        self.Lp_norm_power = Lp_norm_power
        self.reduce_results = reduce_results
        self._maps = {}

    @staticmethod
    def _axis_vector(n, nq):
        q, w = np.polynomial.legendre.leggauss(nq)
        q32, w32 = q.astype(np.float32), w.astype(np.float32)
        step = np.float32(2.0 / (n - 1))
        pos = (q32 + np.float32(1.0)) / step                       # integral_loss.py:7-9 in float32
        lo, hi = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
        hi = np.where(hi == lo, hi + 1, hi)                           # :11-14
        grid = np.linspace(-1.0, 1.0, n)
        t = (q32.astype(np.float64) - grid[lo]) / (grid[hi] - grid[lo])
        v = np.zeros(n)
        np.add.at(v, lo, w32.astype(np.float64) * (1.0 - t))
        np.add.at(v, hi, w32.astype(np.float64) * t)
        return v

    def _axis_on_device(self, n, nq, device):
        key = (n, nq, str(device))
        v = self._maps.get(key)
        if v is None:
            v = self._maps[key] = ops.upload(self._axis_vector(n, nq), device)      # float64, n values
        return v

    def weight_map(self, H, W, device):
        """G = outer(v_H, v_W): the product in float64 rounded once to float32 - formed on the device from the two cached axis vectors (one tiny
        launch per call).  Keeping a whole (H, W) map per shape, as until round 5, grows without bound under the shipped training workload
        (experiments/hpnn.json: a new grid shape in [192, 384]^2 every batch - 37 k possible shapes x 0.3 MB); the axis vectors are at most a few
        hundred short arrays.  Same bits as the host-side outer product it replaces."""
        return torch.outer(self._axis_on_device(H, self.n_quadpts[0], device), self._axis_on_device(W, self.n_quadpts[1], device)).to(torch.float32)


class loss_wrapper:
    def __init__(self, ndims, integral_loss_weight, integral_loss_config, physics_informed_loss_weight, physics_informed_loss_config,
                 data_format='channels_first', mse_loss_weight=0.0, mae_loss_weight=0.0, scale_sample_loss_by_target_peak_magnitude=False,
                 global_batch_size=None):
        if ndims != 2 or data_format not in ('channels_first', 'channels_last'):
            raise NotImplementedError('loss_wrapper: 2-D only')
        self.ndims, self.data_format = ndims, data_format       # channels_last: the public __call__ takes (N,H,W,1) tensors (one channel: a reshape)
        integral_loss_config = dict(integral_loss_config, data_format='channels_first')
        self.integral_loss_weight = float(integral_loss_weight)
        self.physics_informed_loss_weight = float(physics_informed_loss_weight)
        self.mse_loss_weight, self.mae_loss_weight = float(mse_loss_weight), float(mae_loss_weight)
        self.scale = bool(scale_sample_loss_by_target_peak_magnitude)
        self.global_batch_size = global_batch_size
        icfg = {k: v for k, v in integral_loss_config.items() if k not in ('ndims', 'data_format')}
        self.integral_loss = integral_loss(ndims=ndims, reduce_results=True, **icfg)
        self.lp = float(self.integral_loss.Lp_norm_power)      # exponent of the integral term (integral_loss.py:153) and of its peak scaling (:68)
        pcfg = {k: v for k, v in physics_informed_loss_config.items() if k not in ('ndims', 'data_format')}
        self._init_physics_informed(pcfg, ndims)
        self.pi_normalize = bool(pcfg.get('normalize', False))
        self._last = None

    def _init_physics_informed(self, pcfg, ndims):
        self.pi_stencil = build_fd_coefficients(pcfg.get('stencil_sizes', 5), pcfg.get('orders', 2), ndims)
        self.pi_domain_norm = bool(pcfg.get('inputs_have_max_domain_size_squared_normalization', False))

    # -- helpers
    def _pi_kernels(self, dx, H, W):
        """losses/physics_informed_loss.py:36-42: per-sample stencil sum_d coeff[d] * q[n,d]."""
        st = torch.tensor(self.pi_stencil, dtype=torch.float32, device=dx.device)
        if self.pi_domain_norm:
            sizes = dx * torch.tensor([H - 1.0, W - 1.0], device=dx.device)
            q = (sizes.max(dim=1, keepdim=True).values / dx) ** 2
        else:
            q = 1.0 / dx ** 2
        return torch.einsum('dij,nd->nij', st, q).contiguous()

    def _evaluate(self, y_true, y_pred, rhs, dx, want_grad):
        N, _, H, W = y_pred.shape
        dev = y_pred.device
        y_true = y_true.to(device=dev, dtype=torch.float32).contiguous()
        y_pred = y_pred.contiguous()
        gbs = N if self.global_batch_size is None else int(self.global_batch_size)
        G = self.integral_loss.weight_map(H, W, dev) if self.integral_loss_weight != 0.0 else None
        part = ops.loss_partials(y_pred, y_true, G, self.lp)
        extra = None
        pi = None
        if self.physics_informed_loss_weight != 0.0:
            sums, points, peak, pi = self._pi_partials(y_pred, rhs, dx, H, W)
            coef = torch.full((N,), self.physics_informed_loss_weight / float(N * points), device=dev)
            if self.pi_normalize:
                coef = coef / peak() ** 2
            extra = (coef * sums).sum().reshape(1)
        out = ops.empty((3 * N + 2,), dev)
        loss, mse = out[0:1], out[1:2]
        c_mae, c_mse, c_int = out[2:2 + N], out[2 + N:2 + 2 * N], out[2 + 2 * N:2 + 3 * N]
        ops.handle().call('pcnn_loss_coefficients_p', c_int_(N), c_int64(H * W), ops._p(part), c_float(self.mae_loss_weight), c_float(self.mse_loss_weight),
                          c_float(self.integral_loss_weight), c_float(self.lp), c_int_(1 if self.scale else 0), c_int_(gbs), ops._p(extra), ops._p(loss), ops._p(c_mae),
                          ops._p(c_mse), ops._p(c_int), ops._p(mse))
        self._last = {'mse': mse}
        if not want_grad:
            return loss[0], None
        dpred = ops.loss_bwd(y_pred, y_true, G, c_mae, c_mse, c_int, lp_power=self.lp)
        if pi is not None:
            self._pi_backward(y_pred, pi, coef, dpred)
        return loss[0], dpred

    def _pi_partials(self, y_pred, rhs, dx, H, W):
        """The physics-informed term of one batch -> (per-sample sums of the squared residual, residual points per sample, a callable giving
        max|rhs| per sample, what _pi_backward needs)."""
        rhs = rhs.to(device=y_pred.device, dtype=torch.float32).contiguous()
        kern = self._pi_kernels(dx.to(y_pred.device), H, W)
        sy, sx = kern.shape[-2], kern.shape[-1]
        return ops.pi_loss_partials(y_pred, rhs, kern), (H - 2 * (sy // 2)) * (W - 2 * (sx // 2)), lambda: rhs.abs().amax(dim=(1, 2, 3)), (rhs, kern)

    def _pi_backward(self, y_pred, pi, coef, dpred):
        ops.pi_loss_bwd(y_pred, pi[0], pi[1], coef, dpred)

    def __call__(self, y_true, y_pred, rhs, dx):
        if self.data_format == 'channels_last':
            y_true, y_pred, rhs = [t.reshape((t.shape[0], 1) + tuple(t.shape[1:-1])) if (t is not None and t.dim() == 4) else t for t in (y_true, y_pred, rhs)]
        return self._evaluate(y_true, y_pred, rhs, dx, False)[0]

    def value_and_grad(self, y_true, y_pred, rhs, dx):
        """(loss scalar tensor, dL/dy_pred) - what tape.gradient(loss, y_pred) would give."""
        return self._evaluate(y_true, y_pred, rhs, dx, True)

    def value(self, y_true, y_pred, rhs, dx):
        """The loss scalar of channels-first tensors without the gradient pass (test_step / evaluate); rhs may be None when the
        physics-informed weight is zero."""
        return self._evaluate(y_true, y_pred, rhs, dx, False)[0]

    def mse_metric(self, y_true, y_pred):
        """tf.reduce_mean((pred - ground_truth)**2) of the last evaluated (micro-)batch (train_step :291)."""
        return self._last['mse'][0]


class variable_density_loss_wrapper(loss_wrapper):
    """loss_wrapper for the variable-density problem div((1/rho) grad u) = f.  Same constructor; `rhs` is the (N,2,H,W)
    stack [rhs, rho] of dataset.variable_density_dataset_generator.  The MAE, MSE and integral terms are loss_wrapper's.  The physics-informed
    term is the flux-form residual of the solver's own discretisation (dataset.variable_density_poisson_solve),
        weight / (N (H-2)(W-2)) * sum over samples and interior nodes of (L_rho pred - rhs)^2,     each sample divided by max|rhs|^2 under `normalize`,
    with its gradient w.r.t. the prediction on every node; rho gets none.  The flux form exists for the 5-point stencil only: `stencil_sizes` and
    `orders` are accepted at 3 and 2, `inputs_have_max_domain_size_squared_normalization` at False.  One spacing per sample: dx (N,1), or (N,2) with
    equal columns.  channels_first only.
    boundary_types: None, or a dict edge -> 'dirichlet' | 'neumann' as the solver and the generator take it.  The residual is
    then summed over the unknowns of those edge types - a Neumann edge's nodes included, with the solver's half-cell closure and du/dn = 0 - each
    weighted by w = w_i w_j (1/2 on a Neumann edge's row), and divided by N sum(w); all Dirichlet is today's N (H-2)(W-2)."""

    def __init__(self, *args, boundary_types=None, **kwargs):
        from .utils import neumann_mask
        if boundary_types is not None and not isinstance(boundary_types, dict):
            raise ValueError("variable_density_loss_wrapper: boundary_types is None or a dict edge -> 'dirichlet' | 'neumann', got %r" % (boundary_types,))
        self.boundary_types = boundary_types
        self.neumann_mask = neumann_mask(boundary_types)           # refuses an unknown edge name or type
        super().__init__(*args, **kwargs)

    def weight_sum(self, H, W):
        """sum(w) over the unknowns: (rows - half a row per Neumann left / right edge) x (columns likewise); (H-2)(W-2) for all Dirichlet."""
        m = self.neumann_mask
        if m == 0:
            return (H - 2) * (W - 2)
        return (H - 2 + 0.5 * ((m & 1) + (m >> 1 & 1))) * (W - 2 + 0.5 * ((m >> 2 & 1) + (m >> 3 & 1)))

    def _init_physics_informed(self, pcfg, ndims):
        if self.data_format != 'channels_first':
            raise NotImplementedError('variable_density_loss_wrapper: data_format channels_first only')
        for key, want in (('stencil_sizes', 3), ('orders', 2)):
            if key in pcfg and any(int(v) != want for v in np.atleast_1d(pcfg[key])):
                raise NotImplementedError('variable_density_loss_wrapper: physics_informed_loss_config[%r] = %r - the flux-form residual is the 5-point '
                                          'one (%s = %d)' % (key, pcfg[key], key, want))
        if pcfg.get('inputs_have_max_domain_size_squared_normalization', False):
            raise NotImplementedError("variable_density_loss_wrapper: physics_informed_loss_config['inputs_have_max_domain_size_squared_normalization'] is not "
                                      'implemented for the flux-form residual')

    @staticmethod
    def _check_stack(stack, like):
        if stack is None or stack.dim() != 4 or stack.shape[1] != 2 or tuple(stack.shape[2:]) != tuple(like.shape[2:]) or stack.shape[0] != like.shape[0]:
            raise ValueError('variable_density_loss_wrapper: rhs must be the (N,2,H,W) stack [rhs, rho] matching the prediction %s, got %s'
                             % (tuple(like.shape), None if stack is None else tuple(stack.shape)))

    @staticmethod
    def _spacing(dx, N):
        """dx (N,), (N,1) or (N,2) -> (N,) on dx's device; differing columns are anisotropic spacing, which the solver does not do either."""
        dx = dx.to(torch.float32).reshape(N, -1)
        if dx.shape[1] == 2:
            if not bool((dx[:, 0] == dx[:, 1]).all()):
                raise NotImplementedError('variable_density_loss_wrapper: anisotropic spacing (dy != dx) is not supported')
        elif dx.shape[1] != 1:
            raise ValueError('variable_density_loss_wrapper: dx must be (N,1) or (N,2), got %s' % (tuple(dx.shape),))
        return dx[:, 0].contiguous()

    def _evaluate(self, y_true, y_pred, rhs, dx, want_grad):
        if self.physics_informed_loss_weight != 0.0:
            self._check_stack(rhs, y_pred)                   # refuse a one-channel rhs before any kernel runs (no copy is made here)
        return super()._evaluate(y_true, y_pred, rhs, dx, want_grad)

    def _pi_partials(self, y_pred, rhs, dx, H, W):
        stack = rhs.to(device=y_pred.device, dtype=torch.float32)
        f, rho = stack[:, 0].contiguous(), stack[:, 1].contiguous()
        h = self._spacing(dx.to(y_pred.device), y_pred.shape[0])
        return ops.varcoef_pi_loss_partials(y_pred, rho, f, h, self.neumann_mask), self.weight_sum(H, W), lambda: f.abs().amax(dim=(1, 2)), (f, rho, h)

    def _pi_backward(self, y_pred, pi, coef, dpred):
        ops.varcoef_pi_loss_bwd(y_pred, pi[1], pi[0], pi[2], coef.contiguous(), dpred, self.neumann_mask)


c_int_ = c_int
