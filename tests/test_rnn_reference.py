"""Pins tests/rnn_twin.py (the fp64 restatement of the Keras LSTM / GRU equations) against torch.nn.LSTM / torch.nn.GRU in fp64 - no GPU."""
import pytest
import torch

from tests import rnn_twin as R

TOL = 1e-12


def rel(a, b):
    return float((a - b).norm() / b.norm())


def make(cell, N, T, cin, u, seed=0, bias=True):
    g = torch.Generator().manual_seed(seed)
    G = 4 if cell == 'lstm' else 3
    x = torch.cumsum(torch.randn(N, T, cin, generator=g, dtype=torch.float64), 1) * 0.1
    W = torch.randn(cin, G * u, generator=g, dtype=torch.float64) * 0.3
    U = torch.randn(u, G * u, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn((G * u,) if cell == 'lstm' else (2, G * u), generator=g, dtype=torch.float64) * 0.1 if bias else None
    gy = torch.randn(N, T, u, generator=g, dtype=torch.float64)
    return x, W, U, b, gy


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
@pytest.mark.parametrize('shape', [(3, 17, 1, 5), (2, 40, 6, 11)])
def test_twin_matches_torch_nn(cell, shape):
    N, T, cin, u = shape
    x, W, U, b, gy = make(cell, N, T, cin, u)
    leaves = [t.clone().requires_grad_(True) for t in (x, W, U, b)]
    y = R.layer(cell, *leaves)
    grads = torch.autograd.grad((y * gy).sum(), leaves)
    m = (torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(cin, u, batch_first=True).double()
    wih, whh, bih, bhh = (R.torch_lstm_weights if cell == 'lstm' else R.torch_gru_weights)(W, U, b)
    with torch.no_grad():
        m.weight_ih_l0.copy_(wih); m.weight_hh_l0.copy_(whh); m.bias_ih_l0.copy_(bih); m.bias_hh_l0.copy_(bhh)
    xt = x.clone().requires_grad_(True)
    yt = m(xt)[0]
    (yt * gy).sum().backward()
    assert rel(y.detach(), yt.detach()) <= TOL
    assert rel(grads[0], xt.grad) <= TOL
    if cell == 'lstm':
        assert rel(grads[1], m.weight_ih_l0.grad.t()) <= TOL
        assert rel(grads[2], m.weight_hh_l0.grad.t()) <= TOL
        assert rel(grads[3], m.bias_ih_l0.grad) <= TOL and rel(grads[3], m.bias_hh_l0.grad) <= TOL
    else:
        inv = torch.argsort(R.gru_perm(u))
        assert rel(grads[1], m.weight_ih_l0.grad[inv].t()) <= TOL
        assert rel(grads[2], m.weight_hh_l0.grad[inv].t()) <= TOL
        assert rel(grads[3][0], m.bias_ih_l0.grad[inv]) <= TOL and rel(grads[3][1], m.bias_hh_l0.grad[inv]) <= TOL


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_go_backwards_is_the_twin_on_the_flipped_input(cell):
    x, W, U, b, _ = make(cell, 2, 13, 3, 4, seed=1)
    y = R.layer(cell, x, W, U, b, go_backwards=True)
    assert torch.equal(y, R.layer(cell, torch.flip(x, [1]), W, U, b))               # outputs stay in processing order
    assert rel(y, torch.flip(y, [1])) > 1e-2


def test_hard_sigmoid_formula():
    x = torch.linspace(-4, 4, 33, dtype=torch.float64)
    expect = torch.tensor([min(max(0.2 * float(v) + 0.5, 0.0), 1.0) for v in x], dtype=torch.float64)
    assert torch.equal(R.hard_sigmoid(x), expect)
    xs, W, U, b, _ = make('lstm', 2, 9, 2, 3, seed=2)
    assert rel(R.lstm(xs, W, U, b, rec='hard_sigmoid'), R.lstm(xs, W, U, b)) > 1e-3


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_use_bias_false_is_a_zero_bias(cell):
    x, W, U, b, _ = make(cell, 2, 11, 2, 5, seed=3)
    assert rel(R.layer(cell, x, W, U, None), R.layer(cell, x, W, U, torch.zeros_like(b))) <= TOL
    assert rel(R.layer(cell, x, W, U, None), R.layer(cell, x, W, U, b)) > 1e-3


def test_wrong_twins_differ():
    x, W, U, b, _ = make('lstm', 2, 12, 2, 5, seed=4)
    assert rel(R.lstm(x, W, U, b, wrong='swap_if'), R.lstm(x, W, U, b)) > 1e-2
    assert rel(R.lstm(x, W, U, b, go_backwards=True, wrong='flip_back'), R.lstm(x, W, U, b, go_backwards=True)) > 1e-2
    x, W, U, b, _ = make('gru', 2, 12, 2, 5, seed=4)
    assert rel(R.gru(x, W, U, b, wrong='reset_before'), R.gru(x, W, U, b)) > 1e-3
