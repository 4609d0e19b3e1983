"""GRU and tied-weight language models, the CPU half: `mtl_amd.lm.RNNModel('GRU' | 'LSTM', ..., tie_weights)` draws the reference's
initial parameters and lists its names (tests/golden/LG0.npz, recorded from the REAL reference by tools/make_golden_lm_gru.py), the
restatement tests/gru_ref.py that the GPU tests compare against reproduces the reference's logits and state, and its hand-written
cell backward agrees with autograd through torch's nn.GRU in fp64."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gru_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_lg0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'LG0.npz'))
    return z, json.loads(bytes(z['spec']).decode())


def _sha(model):
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()


def _hidden(z, key, name):
    hs = [torch.from_numpy(z['%s/%s_%d' % (key, name, i)]) for i in range(2) if '%s/%s_%d' % (key, name, i) in z.files]
    return tuple(hs) if len(hs) == 2 else hs[0]


@pytest.mark.parametrize('key', ['gru', 'gru_tied', 'lstm_tied'])
def test_model_draws_the_reference_bits_and_the_restatement_matches_its_outputs(key):
    import mtl_amd
    z, spec = load_lg0()
    ms = spec['models'][key]
    torch.set_num_threads(8)
    torch.manual_seed(spec['seed'])
    model = mtl_amd.lm.RNNModel(ms['rnn_type'], spec['ntoken'], ms['ninp'], ms['nhid'], spec['nlayers'], 0.5, ms['tied'])
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(s) for s in z[key + '/param_names']]
    assert list(model.state_dict().keys()) == [str(s) for s in z[key + '/state_keys']]
    assert _sha(model) == bytes(z[key + '/theta0_sha256']).decode()          # same draws, same order as lm/model/rnn_model.py
    assert model._layout.order == names and ('decoder.weight' in model._layout.entries) == (not ms['tied'])
    h0 = model.init_hidden(spec['B'])
    assert torch.is_tensor(h0) == (ms['rnn_type'] == 'GRU')
    assert tuple((h0 if torch.is_tensor(h0) else h0[0]).shape) == (spec['nlayers'], spec['B'], ms['nhid'])
    # the restatement at the same parameters against the recorded eval-mode batch of the reference: fp32 rounding only
    ref = GR.RNNModel(ms['rnn_type'], spec['ntoken'], ms['ninp'], ms['nhid'], spec['nlayers'], 0.5, ms['tied'])
    ref.load_state_dict(model.state_dict())
    assert (ref.decoder.weight is ref.encoder.weight) == ms['tied']
    with torch.no_grad():
        out, hn = ref(torch.from_numpy(z['x']), _hidden(z, key, 'h0'))
    want = _hidden(z, key, 'hn')
    assert float((out - torch.from_numpy(z[key + '/out'])).abs().max()) < 2e-6
    for a, b in zip((hn,) if torch.is_tensor(hn) else hn, (want,) if torch.is_tensor(want) else want):
        assert float((a - b).abs().max()) < 1e-6


@pytest.mark.parametrize('rnn_type', ['GRU', 'LSTM'])
def test_tied_models(rnn_type):
    import mtl_amd
    torch.manual_seed(7)
    model = mtl_amd.lm.RNNModel(rnn_type, 50, 16, 16, 2, 0.2, tie_weights=True)
    assert model.decoder.weight is model.encoder.weight
    assert 'decoder.weight' not in model._layout.entries and 'encoder.weight' in model._layout.entries
    assert [n for n, _ in model.named_parameters()].count('encoder.weight') == 1
    # one tensor inside the flat buffer under both names
    assert model.encoder.weight.data_ptr() == model._layout.view(model.flat_parameters, 'encoder.weight').data_ptr()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert 'decoder.weight' in sd and 'encoder.weight' in sd and torch.equal(sd['decoder.weight'], sd['encoder.weight'])
    torch.manual_seed(8)
    other = mtl_amd.lm.RNNModel(rnn_type, 50, 16, 16, 2, 0.2, tie_weights=True)
    assert not torch.equal(other.flat_parameters, model.flat_parameters)
    other.load_state_dict(sd)                                              # a reference-style tied state dict (both keys)
    assert torch.equal(other.flat_parameters, model.flat_parameters) and other.decoder.weight is other.encoder.weight
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(ValueError, match='nhid must be equal'):
        mtl_amd.lm.RNNModel(rnn_type, 50, 16, 24, 2, 0.2, tie_weights=True)
    with pytest.raises(RuntimeError, match='no CPU'):
        model(torch.zeros(3, 2, dtype=torch.int64), model.init_hidden(2))


def test_other_rnn_types_still_raise():
    import mtl_amd
    for t in ('RNN_TANH', 'RNN_RELU'):
        with pytest.raises(NotImplementedError):
            mtl_amd.lm.RNNModel(t, 50, 16, 16, 2)


def test_gru_entry_points_refuse_bad_arguments_without_a_gpu():
    """the shape limits of the persistent GRU launches are the LSTM's, every entry point returns -22 before any launch, and the
    recordable ones resolve to command-list opcodes"""
    import mtl_amd
    L = mtl_amd._lib.lib()
    for B, H in ((20, 512), (1, 128), (32, 384), (33, 512), (0, 256), (20, 200), (20, 500), (4, 640)):
        assert L.mtl_gru_layer_supported(B, H) == L.mtl_lstm_layer_supported(B, H) == int(1 <= B <= 32 and H in (128, 256, 384, 512))
    assert L.mtl_gru_cell_fwd(None, None, None, None, None, None, None, None, 1.0, 4, 8) == -22
    assert L.mtl_gru_cell_bwd(None, None, None, 1.0, None, None, None, None, None, None, None, 4, 8) == -22
    assert L.mtl_gru_layer_fwd(None, None, None, None, None, None, None, None, 1.0, 5, 20, 512, None) == -22
    assert L.mtl_gru_layer_bwd(None, None, None, 1.0, None, None, None, None, None, 5, 20, 512, None) == -22
    for name in ('mtl_gru_cell_fwd', 'mtl_gru_cell_bwd', 'mtl_gru_layer_fwd', 'mtl_gru_layer_bwd'):
        assert L.mtl_cmdlist_opcode(name.encode()) >= 0, name


def test_restatement_cell_backward_against_autograd_through_nn_gru():
    """fp64: the step-by-step restatement reproduces nn.GRU (forward and parameter gradients), and the hand-written cell backward
    (the formulas the kernels implement) reproduces autograd through one cell, the carry included"""
    torch.manual_seed(2)
    T, B, E, H, NL = 5, 3, 6, 8, 2
    ref = GR.RNNModel('GRU', 20, E, H, NL, 0.0).double()
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 20, (T, B), generator=g)
    h0 = 0.4 * torch.randn(NL, B, H, generator=g, dtype=torch.float64)
    proj = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    feats, hn = ref.features(x, h0)
    want_out, want_hn = ref.rnn(ref.encoder(x), h0)
    assert float((feats - want_out).detach().abs().max()) < 1e-13 and float((hn - want_hn).detach().abs().max()) < 1e-13
    params = list(ref.rnn.parameters())
    for a, b in zip(torch.autograd.grad((feats * proj).sum(), params), torch.autograd.grad((want_out * proj).sum(), params)):
        assert float((a - b).abs().max()) < 1e-12
    # one cell: d(loss)/d(gx, gh, h_prev) by autograd against the formulas
    gx = torch.randn(B, 3 * H, generator=g, dtype=torch.float64, requires_grad=True)
    gh = torch.randn(B, 3 * H, generator=g, dtype=torch.float64, requires_grad=True)
    hp = torch.randn(B, H, generator=g, dtype=torch.float64, requires_grad=True)
    dh = torch.randn(B, H, generator=g, dtype=torch.float64)
    hnew, acts = GR.gru_cell(gx, gh, hp)
    a_gx, a_gh, a_hp = torch.autograd.grad((hnew * dh).sum(), [gx, gh, hp])
    dgx, dgh, carry = GR.gru_cell_backward(dh, acts.detach(), hp.detach())
    assert float((dgx - a_gx).abs().max()) < 1e-14 and float((dgh - a_gh).abs().max()) < 1e-14
    assert float((carry - a_hp).abs().max()) < 1e-14                        # the direct path into h_prev (dgh W_hh is the other one)
    assert float((dgx[:, 2 * H:] - dgh[:, 2 * H:]).abs().max()) > 1e-3      # the two gate-gradient tensors differ in their last third
