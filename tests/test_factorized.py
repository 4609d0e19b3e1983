"""--is-factorized on the CPU: the device model's init (built on the CPU: no library needed) and the restatement of
tests/factorized_util.py both draw the theta0 of tests/golden/FZ0.npz, recorded from the REAL reference
(tools/make_golden_factorized.py); the restatement reproduces FZ0's labels, losses, meta-gradients and parameters of two --copy-grad
meta-steps at the bars of tests/test_oracle_golden.py; the flat layout, the checkpoint format in both directions, and what the factory
stores and still refuses."""
import gzip
import hashlib

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import factorized_util as FU
from tests import golden_util as gu


def _theta_hash(model):
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()


def test_fixture_is_the_configuration_the_tests_assume():
    z, cfg, spec = gu.load('FZ0')
    assert cfg == dict(num_enc_layers=1, num_dec_layers=1, num_heads=8, dim_model=128, dim_key=16, dim_value=16, dim_inner=128, dim_emb=128,
                       src_max_len=500, tgt_max_len=100, r=100, vocab_size=64)
    assert (spec['k'], spec['T'], spec['L'], spec['n_tasks'], spec['iters'], spec['variable']) == (2, 64, 8, 3, 2, True)
    shapes = {str(n): int(z['theta0/%s/numel' % n]) for n in z['param_names']}
    assert shapes['encoder.input_linear_a.weight'] == 100 * 5120 and shapes['encoder.input_linear_b.weight'] == 128 * 100
    assert shapes['encoder.input_linear_b.bias'] == 128 and 'encoder.input_linear.weight' not in shapes
    for pre in ('encoder.layers.0.pos_ffn.', 'decoder.layers.0.pos_ffn.'):
        assert [shapes[pre + n] for n in ('linear_1_a.weight', 'linear_1_b.weight', 'linear_1_b.bias', 'linear_2_a.weight', 'linear_2_b.weight',
                                          'linear_2_b.bias')] == [12800, 12800, 128, 12800, 12800, 128]
        assert pre + 'linear_1_a.bias' not in shapes and pre + 'linear_2_a.bias' not in shapes and pre + 'linear_1.weight' not in shapes


def test_device_model_init_has_the_fixtures_theta0():
    z, cfg, spec = gu.load('FZ0')
    model, vocab, args = FU.device_model(cfg, spec, cuda=False)
    assert model.is_factorized and model.r == 100 and model.encoder.is_factorized and model.decoder.layers[0].is_factorized
    assert [n for n, _ in model.named_parameters()] == [str(s) for s in z['param_names']]
    assert _theta_hash(model) == bytes(z['theta0_sha256']).decode()
    for nm, p in model.named_parameters():
        gu.check_digest(z, 'theta0', nm, p, rtol=0, what='FZ0')
    m = FU.build_model(cfg, seed=1)                          # the state dict loads into the restatement: one format
    m.load_state_dict(model.state_dict())
    assert _theta_hash(m) == _theta_hash(model)


def test_restatement_init_draw_order_bit_identical():
    z, cfg, spec = gu.load('FZ0')
    m = FU.build_model(cfg)
    assert [n for n, _ in m.named_parameters()] == [str(s) for s in z['param_names']]
    assert _theta_hash(m) == bytes(z['theta0_sha256']).decode()


def test_restatement_meta_steps_match_reference():
    """the bars of tests/test_oracle_golden.py::test_meta_step_matches_reference for F0, both iterations"""
    torch.set_num_threads(8)
    z, cfg, spec = gu.load('FZ0')
    m = FU.build_model(cfg)
    names = [n for n, _ in m.named_parameters()]
    adam = R.AdamState(list(m.parameters()), spec['meta_lr'])
    for it in range(spec['iters']):
        tr, val = gu.batches_for(cfg, spec, it, z['data_call_index'])
        G, trl, val_l, labels = R.meta_step(m, adam, tr, val, spec['lr'])
        for j, (gold, hyp) in enumerate(labels):
            key = 'fwd/%d/%d' % (it, j)
            assert np.array_equal(gold.numpy(), z[key + '/gold']) and np.array_equal(hyp.numpy(), z[key + '/hyp']), key
        for j, v in enumerate(v for pair in zip(trl, val_l) for v in pair):
            assert abs(v - float(z['fwd/%d/%d/loss' % (it, j)])) <= 2e-6 * abs(v)
        floor = 1e-4 * gu.global_l2(z, 'G/%d' % it, names)
        for nm, g in zip(names, G):
            gu.check_digest(z, 'G/%d' % it, nm, g, rtol=2e-5, what='FZ0', floor=floor)
        # theta after Adam, at test_oracle_golden's 1e-6 -- on the elements where Adam is well conditioned.  Its step is lr m / (sqrt(v) + eps),
        # d step / d g = lr eps / (|g| + eps)^2 at the first step.  Two summation orders differ by dg ~ 1e-7 of the summands' scale (the
        # tensors' typical |g| is 1e-2 here: dg ~ 1e-9); an element moves by 1e-6 of its own size (~0.05) when lr eps dg / (|g| + eps)^2
        # reaches 5e-8, i.e. below |g| ~ 5e-7.  The factorized block has such elements where F0's dense one has none (linear_2_a's columns
        # of nearly dead inner units: one element of the digest has g = -1.7e-8 and moves by 2e-6).  test_oracle_golden skips tensors of
        # that kind whole; here the digest's elements with |g| < 1e-6 in any iteration so far are left out.
        for nm, p in zip(names, m.parameters()):
            if float(z['G/%d/%s/l2' % (it, nm)]) < floor * 1e-2:     # (Adam on the rounding noise of an exactly-zero gradient: see test_oracle_golden)
                continue
            kind = 'full' if 'theta/%d/%s/full' % (it + 1, nm) in z.files else 'sample'
            ref = z['theta/%d/%s/%s' % (it + 1, nm, kind)].astype(np.float64)
            got = p.detach().numpy().reshape(-1)
            got = (got if kind == 'full' else got[::int(z['theta/%d/%s/step' % (it + 1, nm)])][:ref.size]).astype(np.float64)
            ok = np.ones(ref.shape, bool)
            for j in range(it + 1):
                ok &= np.abs(z['G/%d/%s/%s' % (j, nm, kind)]) >= 1e-6
            assert ok.any(), nm
            err = np.sqrt(((ref - got)[ok] ** 2).sum()) / np.sqrt((ref[ok] ** 2).sum())
            assert err <= 1e-6, (it, nm, err)


def test_gate_replay_of_the_restatement_reproduces_its_free_run():
    """FactorizedFFN honours gates[tag + 'h1'] like refimpl.FFN: replaying the oracle's own decisions gives the free-running output"""
    from oracle import branches
    z, cfg, spec = gu.load('FZ0')
    m = FU.build_model(cfg)
    x, lens, y = gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][0]
    with torch.no_grad():
        (pred, gold, hyp), pre = branches.oracle_trace(m, x, lens, y)
        assert set(k for k in pre if k.endswith('.ff')) == {'e0.ff', 'd0.ff'} and pre['e0.ff'].shape[-1] == cfg['dim_inner']
        pred_g, _, hyp_g = m(x, lens, y, gates=branches.gates_from_oracle_trace(pre))
    assert torch.equal(pred, pred_g) and torch.equal(hyp, hyp_g)


@pytest.mark.parametrize('feat_extractor', ['vgg_cnn', 'large_cnn'])
def test_group_bounds_tile_the_factorized_layout(feat_extractor):
    _, cfg, spec = gu.load('FZ0')
    model, _, args = FU.device_model(cfg, spec, cuda=False, feat_extractor=feat_extractor)
    assert args.dim_input == (5120 if feat_extractor == 'vgg_cnn' else 2560)
    L = model._layout
    gb = L.group_bounds()
    assert list(gb) == ['encoder', 'decoder', 'conv']
    assert gb['encoder'][0] == 0 and gb['encoder'][1] == gb['decoder'][0] and gb['decoder'][1] == gb['conv'][0] and gb['conv'][1] == L.total
    for nm in L.order:                                           # every parameter inside its group's slice, 16-byte aligned
        lo, hi = gb[nm.split('.')[0]]
        assert lo <= L.off(nm) and L.off(nm) + L.entries[nm][2] <= hi and L.off(nm) % 4 == 0
    import mtl_amd
    n_train, n_fixed = mtl_amd.compute_num_params(model)
    assert n_fixed == 0 and n_train == sum(L.entries[nm][2] for nm in L.order)
    assert L.entries['encoder.input_linear_a.weight'][1] == (100, args.dim_input)


def test_factorized_combines_with_logfbank_and_large_cnn_with_logfbank_still_raises():
    import mtl_amd
    _, cfg, spec = gu.load('FZ0')
    vocab = mtl_amd.synthetic_vocab(64)
    a = FU.device_args(cfg, spec, cuda=False, feat='logfbank')
    m = mtl_amd.init_transformer_model(a, vocab, is_factorized=True, r=36)
    assert a.dim_input == 2560 and tuple(m.encoder.input_linear_a.weight.shape) == (36, 2560) and m.r == 36
    with pytest.raises(NotImplementedError, match='logfbank'):
        mtl_amd.init_transformer_model(FU.device_args(cfg, spec, cuda=False, feat='logfbank', feat_extractor='large_cnn'), vocab, is_factorized=True)
    with pytest.raises(NotImplementedError):
        mtl_amd.init_transformer_model(FU.device_args(cfg, spec, cuda=False, feat_extractor='emb_cnn'), vocab, is_factorized=True)


def test_emb_trg_sharing_builds_and_is_stored():
    import mtl_amd
    _, cfg, spec = gu.load('FZ0')
    vocab = mtl_amd.synthetic_vocab(64)
    for fz in (False, True):
        torch.manual_seed(123456)
        shared = mtl_amd.init_transformer_model(FU.device_args(cfg, spec, cuda=False, emb_trg_sharing=True), vocab, is_factorized=fz)
        torch.manual_seed(123456)
        plain = mtl_amd.init_transformer_model(FU.device_args(cfg, spec, cuda=False, emb_trg_sharing=False), vocab, is_factorized=fz)
        assert shared.decoder.emb_trg_sharing is True and plain.decoder.emb_trg_sharing is False
        assert _theta_hash(shared) == _theta_hash(plain)         # only stored (modules/decoder.py:32): the same parameters


@pytest.mark.parametrize('kind', ['meta', 'joint'])
def test_checkpoint_round_trips_the_switch_and_the_tensors(tmp_path, kind):
    import mtl_amd
    _, cfg, spec = gu.load('FZ0')
    model, vocab, args = FU.device_model(cfg, spec, cuda=False, save_folder=str(tmp_path), r=36)
    del args.is_factorized, args.r                               # the saver records how the model was built
    outer = torch.optim.Adam(model.parameters(), lr=1e-3)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.01)
    outer.step()
    if kind == 'meta':
        path = mtl_amd.save_meta_model(model, vocab, 2, torch.optim.SGD(model.parameters(), lr=1e-2), outer, {'avg_valid_cer': 1.0}, args)
        m2, _, _, outer2, epoch, _, a2 = mtl_amd.load_meta_model(path)
    else:
        args.lr = 1e-3
        path = mtl_amd.save_joint_model(model, vocab, 2, outer, {'avg_valid_cer': 1.0}, args)
        m2, _, outer2, epoch, _, a2 = mtl_amd.load_joint_model(path)
    assert epoch == 2 and a2.is_factorized is True and a2.r == 36 and m2.is_factorized and m2.r == 36
    assert [n for n, _ in m2.named_parameters()] == [n for n, _ in model.named_parameters()]
    assert _theta_hash(m2) == _theta_hash(model)
    assert len(outer2.state_dict()['state']) == len(list(model.parameters()))
    assert ('utils.data', 'Vocab') in gu.pickle_globals(path)    # still the reference's class path: both stacks read the file


def test_reference_written_factorized_checkpoint_loads(tmp_path):
    """tests/golden/FZ0.th.gz: save_meta_model of the reference on a tiny factorized model (tools/make_golden_factorized.py)"""
    import mtl_amd
    path = str(tmp_path / 'theirs.th')
    with gzip.open(gu.os.path.join(gu.ROOT, 'tests', 'golden', 'FZ0.th.gz'), 'rb') as f, open(path, 'wb') as g:
        g.write(f.read())
    model, vocab, inner, outer, epoch, metrics, args = mtl_amd.load_meta_model(path)
    assert epoch == 4 and args.is_factorized is True and args.r == 8 and metrics == {'avg_valid_cer': 1.5}
    assert model.is_factorized and model.r == 8 and tuple(model.encoder.input_linear_a.weight.shape) == (8, 5120)
    from mtl_amd import functions
    ck = functions.load_checkpoint_dict(path)
    assert list(ck['model_state_dict']) == list(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), ck['model_state_dict'][k]), k
    # the weights are the tool's exact patterns moved by one Adam step of 1e-3 against a positive gradient
    for i, p in enumerate(model.parameters()):
        ref = (((torch.arange(p.numel()) + 3 * i) % 8).float() - 3.5).view_as(p) / 64 + i / 1024
        assert float((p.detach().cpu() - (ref - 1e-3)).abs().max()) < 1e-6, i
    assert len(outer.state_dict()['state']) == len(list(model.parameters())) and len(vocab.label2id) == 64
