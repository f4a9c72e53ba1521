"""The tape: `torch.autograd` over the libpcnn layers (VERDICT r4 missing #3).

The reference differentiates any composition of its layers with `tf.GradientTape` (models/Homogeneous_Poisson_NN_Legacy.py:265-270).  The classes of
`keras_layers` / `models` expose the same arithmetic as a hand-called pair - `layer(inputs, training=True)` keeps what `layer.backward(dy)` needs -
and this module puts that pair behind a `torch.autograd.Function`, so that a user's own model file, composed from the mirrored layers and ordinary
torch glue (`torch.cat`, `+`, `*`, reductions, a torch loss), trains with `loss.backward()` and any `torch.optim` optimizer:

    from poisson_cnn_amd import keras_layers as K
    from poisson_cnn_amd.autograd import Differentiable

    conv = Differentiable(K.apply_advanced_padding_and_call_conv_layer('SYMMETRIC', K.Conv2D(16, 5, activation='tf.nn.leaky_relu')))
    res = Differentiable(K.resnet(2, filters=16, kernel_size=5, activation='tanh', padding_mode='symmetric'))
    y = res(conv(x)) + x_skip                 # torch tensors on the GPU, part of the autograd graph
    loss = (y - target).square().mean()
    loss.backward()                           # conv.weight.grad / res.weight.grad: the layers' flat parameter gradients
    torch.optim.Adam(list(conv.parameters()) + list(res.parameters())).step()

What is wrapped: every class of `keras_layers` (and the closure `apply_advanced_padding_and_call_conv_layer` returns), the metalearning layers with
the same call / backward convention, and whole models (`models.Homogeneous_Poisson_NN_Legacy`, ...: `Differentiable(model)([rhs, dx])`).  No copies:
the module's one parameter `weight` IS the layer's flat parameter bucket (`store.flat_w`: conv / dense / deconv kernels and biases, then all BN
gamma, then all BN beta - `layer.weight_names` gives the order), an in-place optimizer step is seen by the kernels at once, and the gradient handed to
autograd is the bucket `store.flat_g` the kernels wrote.  The arithmetic is the hand-called pair's, kernel for kernel: gradients are bit-identical to
`layer.backward` (tests/test_gpu_autograd.py).

Rules (the same the hand-chained form has): one forward per backward and per layer object - a layer keeps the activations of ONE call, so a module
that is applied twice before `backward()` raises instead of differentiating the wrong call (build two layers, as the reference's models do);
`torch.no_grad()` / `module.eval()` run the inference path (`training=False`: nothing kept, BatchNormalization on its moving statistics).

Also here, and independent of the layers: `variable_density_solve` and `variable_density_residual` put the variable-density Poisson solve and its
flux-form residual on the tape with gradients with respect to their DATA - `rho`, `rhs`, the edge arrays -, and
`variable_density_smooth` does the same for the Jacobi smoother between them (`u`, `rho`, `rhs`; section 25).
"""
import torch

__all__ = ['Differentiable', 'differentiable', 'variable_density_solve', 'variable_density_residual', 'variable_density_smooth']


def _is_float_tensor(v):
    return isinstance(v, torch.Tensor) and v.is_floating_point()


class _Pair(torch.autograd.Function):
    """forward = layer.call(inputs, training=True); backward = layer.backward(dy) + the flat parameter gradient."""

    @staticmethod
    def forward(ctx, module, flat_w, *tensors):
        layer = module.layer
        if module._pending:
            raise RuntimeError('%s was applied twice before backward(): a libpcnn layer keeps the activations of one call - use one layer object per '
                               'application (as the reference\'s models do); if the earlier forward was never differentiated, call module.reset()' % type(layer).__name__)
        out = module._call(module._rebuild(tensors), True)
        if not isinstance(out, torch.Tensor):
            raise TypeError('%s returned %s: only single-tensor outputs are differentiable here' % (type(layer).__name__, type(out).__name__))
        module._pending = True
        ctx.module = module
        ctx.n = len(tensors)
        return out

    @staticmethod
    def backward(ctx, dy):
        module = ctx.module
        layer = module.layer
        module._pending = False
        g = layer.backward(dy.contiguous())
        store = module._store()
        gw = store.flat_g.clone() if (store is not None and ctx.needs_input_grad[1]) else None
        grads = [None] * ctx.n
        if isinstance(g, (list, tuple)):
            for i, gi in zip(module._tensor_slots_differentiable, g):
                grads[i] = gi
        elif g is not None and ctx.n:
            grads[0] = g
            if any(ctx.needs_input_grad[2 + i] for i in range(1, ctx.n)):
                raise RuntimeError('%s.backward returns the gradient of its first tensor input only (as the reference\'s graph needs it); another '
                                   'input of this call requires grad and would silently get none' % type(layer).__name__)
        for i in range(ctx.n):
            if not ctx.needs_input_grad[2 + i]:
                grads[i] = None
        return (None, gw, *grads)


class Differentiable(torch.nn.Module):
    """A libpcnn layer, block or model as a `torch.nn.Module` on the autograd tape (module docstring)."""

    def __init__(self, layer):
        super().__init__()
        if isinstance(layer, Differentiable):
            layer = layer.layer
        fn = None
        if not hasattr(layer, 'backward') or not (hasattr(layer, 'call') or callable(layer)):
            raise TypeError('%r has no call / backward pair' % (layer,))
        if not hasattr(layer, 'call'):                         # the closure of apply_advanced_padding_and_call_conv_layer: layer(x, training=...)
            fn = layer
            if not hasattr(fn, 'layer'):
                raise TypeError('a callable without .layer cannot be wrapped')
            layer = fn.layer
        self.layer = layer
        self._fn = fn
        self._pending = False
        self._warmed = False
        self._tensor_slots_differentiable = [0]
        self._template = None
        self.weight = None                                     # registered at the first call (the layers build lazily, from their first input)

    # -- the layer's parameter bucket
    def _store(self):
        return getattr(self.layer, 'store', None)

    def _call(self, inputs, training):
        return self._fn(inputs, training=training) if self._fn is not None else self.layer.call(inputs, training=training)

    def _bind_parameters(self):
        store = self._store()
        if self.weight is None and store is not None and getattr(store, 'flat_w', None) is not None and store.flat_w.numel() > 0:
            self.weight = torch.nn.Parameter(store.flat_w, requires_grad=True)          # shares the bucket's storage: no copy, in-place updates are seen

    # -- inputs: a tensor, or the reference's list conventions with tensors and plain values mixed
    def _split(self, inputs):
        if isinstance(inputs, (list, tuple)):
            slots = [i for i, v in enumerate(inputs) if _is_float_tensor(v)]
            self._template = ('list', list(inputs), slots)
            return [inputs[i] for i in slots]
        if not _is_float_tensor(inputs):
            inputs = torch.as_tensor(inputs, dtype=torch.float32)
        self._template = ('tensor', None, [0])
        return [inputs]

    def _rebuild(self, tensors):
        kind, vals, slots = self._template
        if kind == 'tensor':
            return tensors[0]
        vals = list(vals)
        for i, t in zip(slots, tensors):
            vals[i] = t
        return vals

    def forward(self, inputs):
        tensors = self._split(inputs)
        if not self._warmed:
            if not getattr(self.layer, 'built', True):         # lazy build (keras_layers): one inference call creates the parameter bucket
                with torch.no_grad():
                    self._call(self._rebuild(tensors), False)
            self._warmed = True
        self._bind_parameters()
        if not (torch.is_grad_enabled() and self.training):
            self._pending = False                              # an inference call replaces whatever an undifferentiated training forward left behind
            with torch.no_grad():
                return self._call(self._rebuild(tensors), False)
        # which tensor inputs the layer's backward returns gradients for: all of them where it returns a list (MergeWithAttention), else the first
        n = len(tensors)
        self._tensor_slots_differentiable = list(range(n))
        w = self.weight if self.weight is not None else torch.zeros(0, device=tensors[0].device if n else 'cpu')
        return _Pair.apply(self, w, *tensors)

    def reset(self):
        """Forgets a training-mode forward that will never be differentiated (a logged loss, an exception before loss.backward()): the next forward is
        accepted again.  The layer's saved activations are simply overwritten by that forward."""
        self._pending = False

    def extra_repr(self):
        return '%s, %d parameters' % (type(self.layer).__name__, 0 if self.weight is None else self.weight.numel())


def differentiable(layer):
    """`Differentiable(layer)`, for use as a decorator-style one-liner around a freshly constructed layer."""
    return Differentiable(layer)


# ----------------------------------------------------------------------------- the variable-density problem, differentiable in its data
_EDGES = ('left', 'right', 'bottom', 'top')


def _like(grad, t):
    """A gradient computed on the solver's normalised layout, in the shape and dtype of the input it belongs to (a batch of 1 that was broadcast: summed)."""
    if grad.numel() != t.numel():
        grad = grad.reshape(grad.shape[0], -1).sum(0)
    return grad.reshape(t.shape).to(t.dtype)


class _VariableDensitySolve(torch.autograd.Function):
    """forward = dataset.variable_density_poisson_solve; backward = one adjoint solve with the same solver, then the gathers of csrc/varcoef_grad.hip."""

    @staticmethod
    def forward(ctx, rho, rhs, left, right, bottom, top, dx, opts, adjoint_tol, initial_guesses):
        from . import dataset as D
        edges = dict(zip(_EDGES, (left, right, bottom, top)))
        soln = D.variable_density_poisson_solve(rho, rhs, edges, dx, initial_guesses=initial_guesses, **opts)
        ctx.opts, ctx.adjoint_tol = opts, adjoint_tol
        ctx.save_for_backward(rho, rhs, left, right, bottom, top, dx, soln)
        return soln

    @staticmethod
    def backward(ctx, dy):
        from . import dataset as D, ops
        from .dataset import _kernels as K
        rho, rhs, left, right, bottom, top, dx, soln = ctx.saved_tensors
        inputs = (rho, rhs, left, right, bottom, top)
        need = ctx.needs_input_grad[:6]
        N, _, H, W = soln.shape
        neumann = D.neumann_flags(ctx.opts['boundary_types']) if ctx.opts['boundary_types'] is not None else (False,) * 4
        mask = sum(int(f) << k for k, f in enumerate(neumann))
        r, b, d, dev = D._solver_args(rhs.detach(), {k: v.detach() for k, v in zip(_EDGES, inputs[2:])}, dx.detach(), soln.device)
        dens = rho.detach().to(device=dev, dtype=torch.float32).reshape(N, H, W).contiguous()
        # A^T lam = du on the unknowns.  W A is symmetric: A mu = W^-1 du, lam = W mu - the solver's own system with the right-hand side field
        # -W^-1 du (its b is -f) and zero edge data, cold start.  An adjoint that has not converged raises the solver's RuntimeWarning.
        du = dy.detach().to(torch.float32).reshape(N, H, W).contiguous()
        (i0, i1), (j0, j1) = K.varcoef_unknowns(H, W, neumann)
        wi, wj = K.varcoef_weights(H, W, neumann, dev)
        w = torch.zeros((H, W), dtype=torch.float32, device=dev)
        w[i0:i1 + 1, j0:j1 + 1] = (wi[:, None] * wj[None, :]).to(torch.float32)
        winv = torch.where(w > 0, 1.0 / w.clamp_min(0.25), w)                    # 1, 2 or 4: exact
        zero = {k: torch.zeros_like(b[k]) for k in _EDGES}
        mu = D.variable_density_poisson_solve(dens, -(du * winv), zero, d, **dict(ctx.opts, tol=ctx.adjoint_tol))
        lam = (mu.reshape(N, H, W) * w).contiguous()
        grads = [None] * 6
        if need[0]:
            grads[0] = _like(ops.varcoef_coef_grad(lam, soln.reshape(N, H, W), dens, d, mask, {k: b[k] for k, f in zip(_EDGES, neumann) if f}), rho)
        if need[1]:
            grads[1] = _like(-lam, rhs)
        if any(need[2:]):
            for i, g in enumerate(ops.varcoef_edge_grad(lam, dens, d, mask, du)):
                if need[2 + i]:
                    grads[2 + i] = _like(g, inputs[2 + i])
        return (*grads, None, None, None, None)


def variable_density_solve(rho, rhs, boundaries, dx, boundary_types=None, tol=1e-10, max_iterations=500, check_every=8, preconditioner='dst',
                           initial_guesses=None, adjoint_tol=None):
    """`dataset.variable_density_poisson_solve` on the `torch.autograd` tape: the (N,1,H,W) float32 solution of div((1/rho) grad u) = rhs, bit for bit
    the solver's, differentiable with respect to `rho`, `rhs` and the four arrays of `boundaries` (Dirichlet values or Neumann du/dn) - whichever of
    them `requires_grad`.  Tensors on the device in the solver's shapes; `dx` and `initial_guesses` get no gradient.

    backward is one more solve of the same system (same rho, dx, boundary_types, preconditioner, max_iterations, check_every; tolerance `adjoint_tol`,
    default `tol`; cold start) for the adjoint variable lam, then two gather kernels (ops.varcoef_coef_grad, ops.varcoef_edge_grad; d rhs = -lam).
    An adjoint solve that has not converged raises the solver's RuntimeWarning.  Without an input that requires grad, or under torch.no_grad(),
    nothing but the forward solve runs.  Refused: all four edges Neumann (the singular system the solver projects and shifts), and the solver's own
    refusals (anisotropic spacing among them)."""
    from . import dataset as D
    if boundary_types is not None and all(D.neumann_flags(boundary_types)):
        raise NotImplementedError('variable_density_solve: the all-Neumann problem is singular (the solver projects the data and fixes the mean); '
                                  'its derivative is not built - use variable_density_poisson_solve for the solution itself')
    missing = [k for k in _EDGES if k not in boundaries]
    if missing:
        raise ValueError('boundaries lacks %r' % (missing,))
    for name, t in (('rho', rho), ('rhs', rhs), ('dx', dx)) + tuple((k, boundaries[k]) for k in _EDGES):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError('variable_density_solve: %s must be a tensor on the device' % name)
    opts = dict(tol=float(tol), max_iterations=int(max_iterations), check_every=int(check_every), preconditioner=preconditioner, boundary_types=boundary_types)
    return _VariableDensitySolve.apply(rho, rhs, boundaries['left'], boundaries['right'], boundaries['bottom'], boundaries['top'], dx, opts,
                                       float(tol if adjoint_tol is None else adjoint_tol), initial_guesses)


class _VariableDensityResidual(torch.autograd.Function):
    """forward = ops.varcoef_pi_loss_partials; backward = ops.varcoef_pi_loss_bwd (pred) and ops.varcoef_pi_loss_bwd_inputs (the stack)."""

    @staticmethod
    def forward(ctx, pred, stack, dx, mask):
        from . import ops
        p = pred.detach().contiguous()
        rhs, rho, d = stack.detach()[:, 0].contiguous(), stack.detach()[:, 1].contiguous(), dx.detach().reshape(dx.shape[0], -1)[:, 0].contiguous()
        ctx.mask = mask
        ctx.save_for_backward(p, rhs, rho, d)
        return ops.varcoef_pi_loss_partials(p, rho, rhs, d, mask)

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        p, rhs, rho, d = ctx.saved_tensors
        coef = dout.detach().to(torch.float32).contiguous()
        dpred = dstack = None
        if ctx.needs_input_grad[0]:
            dpred = ops.varcoef_pi_loss_bwd(p, rho, rhs, d, coef, torch.zeros_like(p), ctx.mask)        # the kernel accumulates
        if ctx.needs_input_grad[1]:
            dstack = torch.stack(ops.varcoef_pi_loss_bwd_inputs(p, rho, rhs, d, coef, ctx.mask), dim=1)
        return dpred, dstack, None, None


def variable_density_residual(pred, stack, dx, boundary_types=None):
    """(N,) the physics-informed residual sums `ops.varcoef_pi_loss_partials(pred, rho, rhs, dx, mask)` - sum over the unknowns of w (L_rho pred - rhs)^2
    - on the tape: `pred` (N,1,H,W) or (N,H,W), `stack` (N,2,H,W) = [rhs, rho] as the generator hands it out, `dx` (N,), (N,1) or (N,2) (the first
    column), CUDA float32.  The gradient w.r.t. `pred` is ops.varcoef_pi_loss_bwd into zeros, that w.r.t. both channels of `stack` comes from one fused
    launch (ops.varcoef_pi_loss_bwd_inputs).  boundary_types: dict edge -> 'dirichlet' | 'neumann' (None: all Dirichlet); every mask is allowed."""
    from . import dataset as D
    if not isinstance(stack, torch.Tensor) or stack.dim() != 4 or stack.shape[1] != 2:
        raise ValueError('variable_density_residual: stack must be (N,2,H,W) = [rhs, rho], got %r' % (tuple(getattr(stack, 'shape', ())),))
    neumann = D.neumann_flags(boundary_types) if boundary_types is not None else (False,) * 4
    return _VariableDensityResidual.apply(pred, stack, dx, sum(int(f) << k for k, f in enumerate(neumann)))


class _VariableDensitySmooth(torch.autograd.Function):
    """forward = ops.varcoef_jacobi; backward = one ops.varcoef_jacobi_bwd_inputs for the inputs that need a gradient."""

    @staticmethod
    def forward(ctx, u, rho, rhs, d, n_sweeps, mask):
        from . import ops
        N, H, W = ops._one_channel_shape('variable_density_smooth', u, 'fields must be (N,H,W), (N,1,H,W) or (N,H,W,1)')
        f = [t.detach().reshape(N, H, W).contiguous() for t in (u, rho, rhs)]
        ctx.n_sweeps, ctx.mask, ctx.shapes = n_sweeps, mask, tuple(t.shape for t in (u, rho, rhs))
        ctx.save_for_backward(*f, d)
        return ops.varcoef_jacobi(*f, d, n_sweeps, mask).reshape(u.shape)

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        u, rho, rhs, d = ctx.saved_tensors
        want = tuple(k for k, need in zip(('u', 'rho', 'rhs'), ctx.needs_input_grad[:3]) if need)
        grads = (None, None, None)
        if want:
            g = dout.detach().to(torch.float32).reshape(u.shape).contiguous()
            grads = ops.varcoef_jacobi_bwd_inputs(g, u, rho, rhs, d, ctx.n_sweeps, ctx.mask, want=want)
        return tuple(None if g is None else g.reshape(s) for g, s in zip(grads, ctx.shapes)) + (None, None, None)


def variable_density_smooth(u, rho, rhs, dx, n_sweeps, boundary_types=None):
    """`ops.varcoef_jacobi(u, rho, rhs, dx, n_sweeps, mask)` on the tape, bit for bit: n_sweeps Jacobi sweeps of div((1/rho) grad u) = rhs from `u`,
    differentiable with respect to `u`, `rho` and `rhs` - whichever of them `requires_grad`.  The fields are CUDA float32,
    (N,H,W), (N,1,H,W) or (N,H,W,1), all with the same points; the result has the shape of `u`.  `dx` (N,), (N,1) or (N,2) with equal columns gets no
    gradient.  boundary_types: dict edge -> 'dirichlet' | 'neumann' (None: all Dirichlet); every mask is allowed.

    backward is one call of ops.varcoef_jacobi_bwd_inputs: the fused adjoint alone when only `u` needs a gradient; otherwise the n_sweeps iterates
    are recomputed into the handle's scratch ((n_sweeps + 2) fields) and one gather launch per sweep accumulates d rho and d rhs.  Refused:
    anisotropic spacing (differing `dx` columns), n_sweeps < 1, and what ops.varcoef_jacobi refuses."""
    from . import dataset as D
    who = 'variable_density_smooth'
    for name, t in (('u', u), ('rho', rho), ('rhs', rhs), ('dx', dx)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError('%s: %s must be a tensor on the device' % (who, name))
    if rho.numel() != u.numel() or rhs.numel() != u.numel():
        raise ValueError('%s: rho %s and rhs %s must have the points of u %s' % (who, tuple(rho.shape), tuple(rhs.shape), tuple(u.shape)))
    if int(n_sweeps) < 1:
        raise ValueError('%s: n_sweeps must be at least 1, got %r' % (who, n_sweeps))
    d = dx.detach().to(torch.float32).reshape(dx.shape[0], -1)
    if d.shape[1] == 2:
        if not bool((d[:, 0] == d[:, 1]).all()):
            raise NotImplementedError('%s: anisotropic spacing (dy != dx) is not supported' % who)
    elif d.shape[1] != 1:
        raise ValueError('%s: dx must be (N,), (N,1) or (N,2), got %s' % (who, tuple(dx.shape)))
    neumann = D.neumann_flags(boundary_types) if boundary_types is not None else (False,) * 4
    return _VariableDensitySmooth.apply(u, rho, rhs, d[:, 0].contiguous(), int(n_sweeps), sum(int(f) << k for k, f in enumerate(neumann)))
