"""feat_extractor='large_cnn' on the CPU: the restatement of tests/large_cnn_util.py reproduces tests/golden/LC0.npz -- theta0, labels,
losses, the meta-gradient and theta1 of one --copy-grad meta-step recorded from the REAL reference (tools/make_golden_large_cnn.py) --
and the device model's init (built on the CPU: no library needed) draws the same theta0; the factory's dim_input and refusals."""
import argparse
import hashlib

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import golden_util as gu
from tests import large_cnn_util as LU


def _theta_hash(model):
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()


def test_fixture_is_the_configuration_the_tests_assume():
    z, cfg, spec = gu.load('LC0')
    assert cfg == dict(num_enc_layers=1, num_dec_layers=1, num_heads=8, dim_model=128, dim_key=16, dim_value=16, dim_inner=128, dim_emb=128,
                       src_max_len=500, tgt_max_len=100, r=100, vocab_size=64)
    assert (spec['k'], spec['T'], spec['L'], spec['n_tasks'], spec['iters'], spec['variable']) == (2, 64, 8, 3, 1, True)
    shapes = {str(n): int(z['theta0/%s/numel' % n]) for n in z['param_names']}
    assert shapes['conv.0.weight'] == 32 * 9 and shapes['conv.2.weight'] == 32 * 32 * 9 and shapes['conv.5.weight'] == 64 * 32 * 9
    assert shapes['conv.7.weight'] == 64 * 64 * 9 and shapes['encoder.input_linear.weight'] == 128 * 2560


def test_restatement_init_draw_order_bit_identical():
    z, cfg, spec = gu.load('LC0')
    m = LU.build_model(cfg)
    assert [n for n, _ in m.named_parameters()] == [str(s) for s in z['param_names']]
    assert _theta_hash(m) == bytes(z['theta0_sha256']).decode()


def test_restatement_meta_step_matches_reference():
    """the bars of tests/test_oracle_golden.py::test_meta_step_matches_reference"""
    torch.set_num_threads(8)
    z, cfg, spec = gu.load('LC0')
    m = LU.build_model(cfg)
    names = [n for n, _ in m.named_parameters()]
    adam = R.AdamState(list(m.parameters()), spec['meta_lr'])
    tr, val = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    G, trl, val_l, labels = R.meta_step(m, adam, tr, val, spec['lr'])
    for j, (gold, hyp) in enumerate(labels):
        assert np.array_equal(gold.numpy(), z['fwd/0/%d/gold' % j]) and np.array_equal(hyp.numpy(), z['fwd/0/%d/hyp' % j]), j
    for j, v in enumerate(v for pair in zip(trl, val_l) for v in pair):
        assert abs(v - float(z['fwd/0/%d/loss' % j])) <= 2e-6 * abs(v)
    floor = 1e-4 * gu.global_l2(z, 'G/0', names)
    for nm, g in zip(names, G):
        gu.check_digest(z, 'G/0', nm, g, rtol=2e-5, what='LC0', floor=floor)
    for nm, p in zip(names, m.parameters()):
        if float(z['G/0/%s/l2' % nm]) < floor * 1e-2:            # (Adam on the rounding noise of an exactly-zero gradient: see test_oracle_golden)
            continue
        gu.check_digest(z, 'theta/1', nm, p, rtol=1e-6, what='LC0')


def test_device_model_init_has_the_fixtures_theta0():
    z, cfg, spec = gu.load('LC0')
    model, vocab, args = LU.device_model(cfg, spec, cuda=False)
    assert args.dim_input == 2560 and model.feat_extractor == 'large_cnn'
    assert [n for n, _ in model.named_parameters()] == [str(s) for s in z['param_names']]
    assert _theta_hash(model) == bytes(z['theta0_sha256']).decode()
    assert [i for i, mod in enumerate(model.conv) if isinstance(mod, torch.nn.Conv2d)] == [0, 2, 5, 7]
    assert [tuple(model.conv[i].weight.shape[:2]) for i in (0, 2, 5, 7)] == [(32, 1), (32, 32), (64, 32), (64, 64)]
    # the state dict loads into the restatement and back: one format
    m = LU.build_model(cfg, seed=1)
    m.load_state_dict(model.state_dict())
    assert _theta_hash(m) == _theta_hash(model)


def test_factory_derives_dim_input_and_refuses_what_is_not_built():
    import mtl_amd
    _, cfg, spec = gu.load('LC0')
    vocab = mtl_amd.synthetic_vocab(64)
    args = LU.device_args(cfg, spec, cuda=False, sample_rate=8000)             # 81 bins -> 20 pooled rows
    mtl_amd.init_transformer_model(args, vocab)
    assert args.dim_input == 20 * 64
    with pytest.raises(NotImplementedError, match='logfbank'):
        mtl_amd.init_transformer_model(LU.device_args(cfg, spec, cuda=False, feat='logfbank'), vocab)
    with pytest.raises(NotImplementedError):
        mtl_amd.init_transformer_model(LU.device_args(cfg, spec, cuda=False, feat_extractor='emb_cnn'), vocab)
    vgg = LU.device_args(cfg, spec, cuda=False, feat_extractor='vgg_cnn')
    mtl_amd.init_transformer_model(vgg, vocab)
    assert vgg.dim_input == 5120


def test_layer_tables():
    from mtl_amd import convstack
    assert [(r.cin, r.cout, r.pool, r.lvl) for r in convstack.LAYERS_LARGE] == [(32, 32, True, 0), (32, 64, False, 1), (64, 64, True, 1)]
    assert [(r.cin, r.cout, r.pool, r.lvl) for r in convstack.LAYERS] == [(64, 64, True, 0), (64, 128, False, 1), (128, 128, True, 1)]
    for a, b in zip(convstack.LAYERS, convstack.LAYERS_LARGE):       # the arena names oracle/branches.py reads
        assert (a.x, a.y, a.am, a.dy, a.dx, a.idx) == (b.x, b.y, b.am, b.dy, b.dx, b.idx)
    eng = argparse.Namespace(conv_h2=True, conv_x3=True, in_linear='h2', conv_layers=convstack.LAYERS_LARGE)
    for h2, x3 in ((True, True), (False, True), (False, False)):
        eng.conv_h2, eng.conv_x3 = h2, x3
        assert convstack.decide(eng, 3, None) == dict(conv_mode='x3', conv_tb=True, in_h2=False)
    eng = argparse.Namespace(conv_h2=True, conv_x3=True, in_linear='h2', conv_layers=convstack.LAYERS)
    assert convstack.decide(eng, 1, None) == dict(conv_mode='h2', conv_tb=False, in_h2=True)
