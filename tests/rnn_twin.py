"""fp64 torch twin of the recurrent layers of Dirichlet_BC_RNN, written from the TF 2.4 Keras equations (an explicit loop over t, autograd for the
gradients), and the model forward on top of it (models/Dirichlet_BC_RNN.py:38-58) with the oracle's resize.  The `wrong` switches build the
deliberately wrong variants the sensitivity tests compare against."""
import torch

from oracle import torch_twin as T


def hard_sigmoid(x):
    return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)


ACTS = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu, 'linear': lambda x: x}
REC = {'sigmoid': torch.sigmoid, 'hard_sigmoid': hard_sigmoid}


def lstm(x, W, U, b=None, act='tanh', rec='sigmoid', go_backwards=False, wrong=None):
    """x (N, T, Cin), W (Cin, 4u), U (u, 4u), b (4u) or None -> h (N, T, u) in processing order.  Gate blocks i, f, c, o."""
    N, Tn, _ = x.shape
    u = U.shape[0]
    a, s = ACTS[act], REC[rec]
    if go_backwards:
        x = torch.flip(x, [1])
    h = x.new_zeros(N, u)
    c = x.new_zeros(N, u)
    out = []
    for t in range(Tn):
        z = x[:, t] @ W + h @ U
        if b is not None:
            z = z + b
        i, f, g, o = z.split(u, 1)
        if wrong == 'swap_if':
            i, f = f, i
        c = s(f) * c + s(i) * a(g)
        h = s(o) * a(c)
        out.append(h)
    y = torch.stack(out, 1)
    return torch.flip(y, [1]) if (go_backwards and wrong == 'flip_back') else y


def gru(x, W, U, b=None, act='tanh', rec='sigmoid', go_backwards=False, wrong=None):
    """reset_after=True: x (N, T, Cin), W (Cin, 3u), U (u, 3u), b (2, 3u) or None.  Blocks z, r, h."""
    N, Tn, _ = x.shape
    u = U.shape[0]
    a, s = ACTS[act], REC[rec]
    if go_backwards:
        x = torch.flip(x, [1])
    h = x.new_zeros(N, u)
    out = []
    for t in range(Tn):
        mx = x[:, t] @ W
        if b is not None:
            mx = mx + b[0]
        xz, xr, xh = mx.split(u, 1)
        if wrong == 'reset_before':                       # reset_after=False arithmetic: the reset gate is applied to h before the recurrent product
            Uz, Ur, Uh = U.split(u, 1)
            bz, br, bh = (b[1].split(u, 0) if b is not None else (0.0, 0.0, 0.0))
            z = s(xz + h @ Uz + bz)
            r = s(xr + h @ Ur + br)
            hh = a(xh + (r * h) @ Uh + bh)
        else:
            mh = h @ U
            if b is not None:
                mh = mh + b[1]
            hz, hr, hhh = mh.split(u, 1)
            z = s(xz + hz)
            r = s(xr + hr)
            hh = a(xh + r * hhh)
        h = z * h + (1.0 - z) * hh
        out.append(h)
    y = torch.stack(out, 1)
    return torch.flip(y, [1]) if (go_backwards and wrong == 'flip_back') else y


def layer(cell, *args, **kw):
    return (lstm if cell == 'lstm' else gru)(*args, **kw)


def forward(model, P, bc, X, wrong=None):
    """model: a poisson_cnn_amd.rnn.Dirichlet_BC_RNN (its structure only); P: name -> fp64 tensor; bc (N, 1, L) fp64 -> (N, 1, X, L)."""
    x = bc.permute(0, 2, 1)                                                 # (N, L, 1): L is the time axis (:45)
    for kn, rn, bn, _, _, act in model.layers:
        x = layer(model.cell, x, P[kn], P[rn], P[bn] if bn is not None else None, act=act, rec=model.rec_act, go_backwards=model.go_backwards)
    img = x.unsqueeze(1)                                                    # (N, 1, L, u_last) (:50)
    L = bc.shape[2]
    out_hw = (L, X) if wrong == 'swap_axes' else (X, L)
    return T.resize2d(img, out_hw, model.resize_method)


def torch_lstm_weights(W, U, b):
    """torch.nn.LSTM parameters of the same layer: same block order, weight_ih = W^T, weight_hh = U^T, bias_ih = b, bias_hh = 0."""
    return W.t().contiguous(), U.t().contiguous(), b.clone(), torch.zeros_like(b)


def gru_perm(u):
    """Keras blocks (z, r, h) -> torch.nn.GRU blocks (r, z, n)."""
    return torch.cat([torch.arange(u, 2 * u), torch.arange(0, u), torch.arange(2 * u, 3 * u)])


def torch_gru_weights(W, U, b):
    p = gru_perm(U.shape[0])
    return W.t()[p].contiguous(), U.t()[p].contiguous(), b[0][p].clone(), b[1][p].clone()
