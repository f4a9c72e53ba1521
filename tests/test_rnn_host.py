"""Dirichlet_BC_RNN (poisson_cnn_amd.rnn <- models/Dirichlet_BC_RNN.py): structure, initialisation, argument handling, checkpoints and the
configuration - no GPU (device='cpu' builds the parameter structure only)."""
import numpy as np
import pytest

from poisson_cnn_amd import configs, tf_checkpoint
from poisson_cnn_amd.rnn import Dirichlet_BC_RNN


def build(**kw):
    cfg = dict(configs.dbcnn_rnn()['model'])
    cfg.update(kw)
    return Dirichlet_BC_RNN(device='cpu', **cfg)


def param_count(units, G, bias_rows):
    """G u (Cin + u) for the two kernels plus the bias: (4u) for the LSTM, (2, 3u) for the GRU with reset_after=True."""
    n, cin = 0, 1
    for u in units:
        n += G * u * (cin + u) + bias_rows * G * u
        cin = u
    return n


def test_param_counts_of_the_shipped_config():
    units = configs.dbcnn_rnn()['model']['units']
    lstm, gru = param_count(units, 4, 1), param_count(units, 3, 2)
    assert lstm == 40800 + 5 * 80400 and gru == 30900 + 5 * 60600
    assert build().count_params() == lstm == 442800
    assert build(RNN_type='GRU').count_params() == gru == 333900
    assert build(use_bias=False).count_params() == param_count(units, 4, 0)


@pytest.mark.parametrize('cell,G', [('lstm', 4), ('gru', 3)])
def test_weight_names_shapes_and_order(cell, G):
    m = build(RNN_type=cell.capitalize(), units=[100, 37, 5])
    expect, shapes, cin = [], [], 1
    for i, u in enumerate([100, 37, 5]):
        s = '_%d' % i if i else ''
        base = '%s%s/%s_cell%s/' % (cell, s, cell, s)
        expect += [base + 'kernel', base + 'recurrent_kernel', base + 'bias']
        shapes += [(cin, G * u), (u, G * u), (G * u,) if cell == 'lstm' else (2, G * u)]
        cin = u
    assert m.weight_names == expect
    assert [w.shape for w in m.get_weights()] == shapes
    assert len(m.trainable_variables) == 9
    lines = []
    m.summary(print_fn=lines.append)
    assert 'Dirichlet_BC_RNN' in lines[0] and str(m.count_params()) in lines[-1]


def test_keras_initialisers():
    m = build(seed=3)
    W = dict(zip(m.weight_names, m.get_weights()))
    for i in range(6):
        s = '_%d' % i if i else ''
        U = W['lstm%s/lstm_cell%s/recurrent_kernel' % (s, s)].astype(np.float64)
        assert np.abs(U @ U.T - np.eye(100)).max() < 1e-5                              # orthogonal over the whole (u, 4u) matrix
        b = W['lstm%s/lstm_cell%s/bias' % (s, s)]
        assert (b[100:200] == 1).all() and (b[:100] == 0).all() and (b[200:] == 0).all()   # unit_forget_bias
        K = W['lstm%s/lstm_cell%s/kernel' % (s, s)]
        lim = np.sqrt(6.0 / (K.shape[0] + K.shape[1]))
        assert np.abs(K).max() <= lim and np.abs(K).max() > 0.9 * lim
    assert (build(unit_forget_bias=False).get_weights()[2] == 0).all()
    g = build(RNN_type='gru')
    assert (g.get_weights()[2] == 0).all() and g.get_weights()[2].shape == (2, 300)
    U = g.get_weights()[1].astype(np.float64)
    assert np.abs(U @ U.T - np.eye(100)).max() < 1e-5
    assert (build(bias_initializer='ones', unit_forget_bias=False).get_weights()[2] == 1).all()
    assert not np.array_equal(build(seed=1).get_weights()[0], build(seed=2).get_weights()[0])


def test_activations_and_units():
    m = build(units=[3, 4], activations=['relu', 'tf.nn.sigmoid'])
    assert m.acts == ['relu', 'sigmoid'] and m.units == [3, 4]
    assert build(activations=None, units=[2]).acts == ['linear']
    assert build(recurrent_activation='hard_sigmoid').rec_act == 'hard_sigmoid'
    for u in (1, 128):
        assert build(units=[u]).count_params() == param_count([u], 4, 1)
    with pytest.raises(NotImplementedError, match='units'):
        build(units=[100, 129])
    with pytest.raises(ValueError):
        build(units=[3, 4], activations=['tanh'])


@pytest.mark.parametrize('kw,name', [
    (dict(dropout=0.1), 'dropout'), (dict(recurrent_dropout=0.2), 'recurrent_dropout'), (dict(stateful=True), 'stateful'), (dict(unroll=True), 'unroll'),
    (dict(return_state=True), 'return_state'), (dict(RNN_type='gru', reset_after=False), 'reset_after'), (dict(time_major=True), 'time_major'),
    (dict(kernel_regularizer='l2'), 'kernel_regularizer'), (dict(kernel_initializer='he_normal'), 'kernel_initializer'),
    (dict(activations=np.tanh), 'activations'), (dict(recurrent_activation=np.tanh), 'recurrent_activation'), (dict(RNN_type=object), 'RNN_type')])
def test_rejected_arguments_raise_with_their_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        build(**kw)


def test_accepted_arguments():
    m = build(RNN_type='gru', recurrent_activation='sigmoid', use_bias=True, go_backwards=True, kernel_initializer='glorot_uniform',
              recurrent_initializer='orthogonal', bias_initializer='zeros', reset_after=True, implementation=1, dropout=0, recurrent_dropout=0.0,
              stateful=False, unroll=False, return_state=False)
    assert m.go_backwards and m.cell == 'gru'
    with pytest.raises(KeyError):
        build(RNN_type='simple')


def test_tf_object_paths():
    m = build(units=[5, 4])
    paths = tf_checkpoint.keras_object_paths(m)
    assert [paths[n] for n in m.weight_names] == ['RNN_layers/%d/cell/%s' % (i, v) for i in range(2) for v in ('kernel', 'recurrent_kernel', 'bias')]
    assert len(tf_checkpoint.keras_object_paths(build(units=[5, 4], use_bias=False))) == 4


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_checkpoint_round_trips(tmp_path, cell):
    a, b = build(RNN_type=cell, units=[7, 3], seed=1), build(RNN_type=cell, units=[7, 3], seed=2)
    a.save_weights(str(tmp_path / 'w.npz'))
    b.load_weights(str(tmp_path / 'w.npz'))
    assert all(np.array_equal(x, y) for x, y in zip(a.get_weights(), b.get_weights()))
    c = build(RNN_type=cell, units=[7, 3], seed=3)
    a.save_weights(str(tmp_path / 'ck'), save_format='tf')
    c.load_weights(str(tmp_path / 'ck'))
    assert all(np.array_equal(x, y) for x, y in zip(a.get_weights(), c.get_weights()))
    with pytest.raises(ValueError):
        build(RNN_type=cell, units=[7, 4]).load_weights(str(tmp_path / 'ck'))


def test_config_restates_the_experiment_file():
    cfg = configs.dbcnn_rnn()
    assert cfg['model'] == {'data_format': 'channels_first', 'activations': 'tanh', 'units': [100] * 6, 'resize_method': 'bilinear', 'RNN_type': 'lstm'}
    assert cfg['dataset'] == {'batch_size': 50, 'batches_per_epoch': 200, 'random_output_shape_range': [[192, 384], [192, 384]], 'random_dx_range': [5e-3, 5e-2],
                              'solver_method': 'multigrid',
                              'boundary_random_smoothness_range': {'left': [3, 8], 'right': [3, 8], 'top': [3, 8], 'bottom': [3, 8]}}
    t = cfg['training']
    assert (t['n_epochs'], t['precision'], t['optimizer'], t['min_learning_rate']) == (200, 'float32', 'adam', 1e-7)
    assert t['optimizer_parameters'] == {'learning_rate': 1e-4, 'amsgrad': False}
    assert t['loss_parameters'] == {'ndims': 2, 'data_format': 'channels_first', 'mae_loss_weight': 1.0, 'integral_loss_weight': 0.4,
                                    'integral_loss_config': {'n_quadpts': 47, 'Lp_norm_power': 2}, 'physics_informed_loss_weight': 0.0,
                                    'physics_informed_loss_config': {'stencil_sizes': [5, 5], 'orders': 2, 'normalize': False},
                                    'scale_sample_loss_by_target_peak_magnitude': False}
    tiny = configs.dbcnn_rnn_tiny()
    assert len(tiny['model']['units']) == 2 and tiny['model']['RNN_type'] == 'lstm'
    Dirichlet_BC_RNN(device='cpu', **tiny['model'])


def test_golden_config_matches(tmp_path):
    """tests/golden/dbcnn_rnn.json is the experiment file's content (settings only); configs.dbcnn_rnn() equals it field by field."""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'dbcnn_rnn.json')) as f:
        assert json.load(f) == configs.dbcnn_rnn()
