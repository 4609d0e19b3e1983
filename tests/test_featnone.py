"""feat_extractor='none' on the CPU: the factory, theta0 and the restatement of tests/featnone_util.py against tests/golden/N0.npz (written
by the real reference: tools/make_golden_featnone.py), the encoder's extent in batchmeta, the argument checks of the entry points of
csrc/mtl_featproj.hip, and -- from tests/x3_emul.py alone -- that every bound tests/test_featnone_gpu.py holds the kernels to separates
six piece products from five."""
import argparse
import hashlib

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import featnone_util as U
from tests import golden_util as gu
from tests import x3_emul as X


def _args(feat_extractor='none', **over):
    _, cfg, spec = gu.load('N0')
    return U.device_args(cfg, spec, feat_extractor=feat_extractor, **over), cfg


@pytest.mark.parametrize('dim_input,feat', [(161, 'spectrogram'), (80, 'logfbank'), (80, 'spectrogram'), (161, 'logfbank')])
def test_factory_accepts_none_and_keeps_dim_input(dim_input, feat, capsys):
    import mtl_amd
    args, cfg = _args(dim_input=dim_input, feat=feat)
    model = mtl_amd.init_transformer_model(args, mtl_amd.synthetic_vocab(cfg['vocab_size']), r=cfg['r'])
    assert args.dim_input == dim_input and tuple(model.encoder.input_linear.weight.shape) == (cfg['dim_model'], dim_input)
    assert model.feat_extractor == 'none' and not hasattr(model, 'conv')
    assert not any(n.startswith('conv.') for n in model.state_dict())
    assert 'the model is initialized without feature extractor' in capsys.readouterr().out
    assert sorted(model._layout.group_bounds()) == ['decoder', 'encoder']


@pytest.mark.parametrize('name', ['emb_cnn', 'None', 'cnn', ''])
def test_other_feature_extractors_still_raise(name):
    import mtl_amd
    args, cfg = _args(name)
    with pytest.raises(NotImplementedError):
        mtl_amd.init_transformer_model(args, mtl_amd.synthetic_vocab(cfg['vocab_size']), r=cfg['r'])


def _theta_hash(model):
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()


def test_theta0_names_and_order_are_the_references():
    z, cfg, spec = gu.load('N0')
    names = [str(s) for s in z['param_names']]
    model, _, _ = U.device_model(cfg, spec)
    assert [n for n, _ in model.named_parameters()] == names and len(names) == 60
    assert sum(p.numel() for p in model.parameters()) == 413440
    assert _theta_hash(model) == bytes(z['theta0_sha256']).decode()
    oracle = U.build_model(cfg)
    assert [n for n, _ in oracle.named_parameters()] == names and _theta_hash(oracle) == bytes(z['theta0_sha256']).decode()
    fz, cfg_fz, spec_fz, d_in = U.load_fz()
    model, _, _ = U.device_model(cfg_fz, spec_fz, dim_input=d_in, is_factorized=True)
    assert [n for n, _ in model.named_parameters()] == [str(s) for s in fz['param_names']]
    assert tuple(model.encoder.input_linear_a.weight.shape) == (cfg_fz['r'], d_in) and model.encoder.input_linear_a.bias is None
    assert _theta_hash(model) == bytes(fz['theta0_sha256']).decode() == _theta_hash(U.build_model(cfg_fz, d_in, True))


def _restatement_meta_steps(z, cfg, spec, m, freq_bins, name):
    """tests/test_oracle_golden.py:test_meta_step_matches_reference, its tolerances"""
    names = [n for n, _ in m.named_parameters()]
    adam = R.AdamState(list(m.parameters()), spec['meta_lr'])
    for it in range(spec['iters']):
        tr, val = U.batches(cfg, spec, it, z['data_call_index'], freq_bins)
        G, trl, val_l, labels = R.meta_step(m, adam, tr, val, spec['lr'])
        for j, (gold, hyp) in enumerate(labels):
            key = 'fwd/%d/%d' % (it, j)
            assert np.array_equal(gold.numpy(), z[key + '/gold']) and np.array_equal(hyp.numpy(), z[key + '/hyp']), key
        for j, v in enumerate(v for pair in zip(trl, val_l) for v in pair):
            assert abs(v - float(z['fwd/%d/%d/loss' % (it, j)])) <= 2e-6 * abs(v)
        floor = 1e-4 * gu.global_l2(z, 'G/%d' % it, names)
        for nm, g in zip(names, G):
            gu.check_digest(z, 'G/%d' % it, nm, g, rtol=2e-5, what=name, floor=floor)
        for nm, p in zip(names, m.parameters()):
            if float(z['G/%d/%s/l2' % (it, nm)]) < floor * 1e-2:
                continue
            gu.check_digest(z, 'theta/%d' % (it + 1), nm, p, rtol=1e-6, what=name)


def test_restatement_reproduces_the_golden():
    torch.set_num_threads(8)
    z, cfg, spec = gu.load('N0')
    assert spec['T'] == 63 and spec['iters'] == 2
    m = U.build_model(cfg)
    tr, _ = U.batches(cfg, spec, 0, z['data_call_index'])
    with torch.no_grad():
        pred, _, _ = m(*tr[0])
    gu.check_digest(z, 'fwd/0/0', 'pred', pred, rtol=2e-5, what='N0')
    _restatement_meta_steps(z, cfg, spec, m, 161, 'N0')


def test_restatement_reproduces_the_factorized_record():
    torch.set_num_threads(8)
    fz, cfg, spec, d_in = U.load_fz()
    _restatement_meta_steps(fz, cfg, spec, U.build_model(cfg, d_in, True), d_in, 'N0 fz')


def test_restatement_reproduces_the_joint_trace_and_the_searches():
    import json
    torch.set_num_threads(8)
    z, cfg, spec = gu.load('N0')
    js = json.loads(bytes(z['joint/spec']).decode())
    m = U.build_model(cfg)
    adam = R.AdamState(list(m.parameters()), js['lr'])
    for it in range(js['iters']):
        tr = [R.synth_batch(1000 * it + 10 * t, js['k'], js['T'], js['L'], cfg['vocab_size'], True) for t in range(js['n_tasks'])]
        _, losses = R.joint_step(m, adam, tr)
        assert np.allclose(losses, z['joint/losses'][it], rtol=2e-6, atol=0), it
    sp = json.loads(bytes(z['decode/spec']).decode())
    m = U.build_model(cfg)
    gu.perturb_output_layer(m.decoder.output_linear.weight, sp)
    x, lens, y = R.synth_batch(sp['seed'], sp['k'], sp['T'], sp['L'], cfg['vocab_size'], True)
    got = R.greedy_search(m, x, lens, R.SOS_ID, sp['greedy_steps'])
    assert np.array_equal(got.numpy().T, z['decode/greedy_ids'])
    labels = ['<PAD>', '<SOS>', '<EOS>', '<OOV>'] + [chr(0x4e00 + i) for i in range(cfg['vocab_size'] - 4)]
    out = R.beam_search(m, x, lens, R.SOS_ID, sp['beam_width'], sp['nbest'], cfg['tgt_max_len'], gu.label_words(labels, labels[:3]))
    assert [seq for utt in out for seq, _ in utt] == [[int(v) for v in r_ if v >= 0] for r_ in z['decode/beam_ids']]


# ---------------------------------------------------------------------------------------------------- the encoder's extent
def _meta(time_shift, T=63, lens=(63, 10), src_max_len=500, **kw):
    from mtl_amd import batchmeta
    y = torch.tensor([[5, 6, 7], [8, 9, 0]])
    kw = dict(kw, time_shift=time_shift) if time_shift is not None else kw
    bm = batchmeta.batch_meta([(torch.tensor(lens, dtype=torch.int32), y)], len(lens), T, src_max_len, 100, **kw)
    f = lambda n, cnt: bm['meta'][bm['off'][n]:bm['off'][n] + cnt]
    return bm, f


def test_extent_of_a_model_without_convolutions():
    from mtl_amd import batchmeta
    assert batchmeta.enc_extent(63, 0) == 63 and batchmeta.enc_extent(63) == 15 == (63 // 2) // 2
    assert all(batchmeta.enc_extent(T) == (T // 2) // 2 for T in range(0, 4100))
    bm, f = _meta(0)
    assert f('klen_enc', 2).tolist() == [63, 10]
    keep = f('keep_enc', 2 * 63).reshape(2, 63)
    assert keep[0].all() and keep[1, :10].all() and not keep[1, 10:].any()
    _meta(0, src_max_len=63)
    with pytest.raises(ValueError, match='positional'):
        _meta(0, src_max_len=62)
    _, f = _meta(0, T=64, lens=(40, 10), frames=[40])                    # stacked at a wider pad: the own width bounds the lengths
    assert f('klen_enc', 2).tolist() == [40, 10] and f('widths', 1).tolist() == [40]
    _meta(0, T=8, lens=(1, 1), frames=[1])                               # one frame is one position
    with pytest.raises(ValueError):
        _meta(2, T=8, lens=(3, 1), frames=[3])                           # behind a conv stack three frames pool to none


def test_extent_of_a_conv_model_is_what_it_was():
    """the same inputs through the default and through time_shift=2: the parent's arrays, written out here"""
    for shift in (None, 2):
        bm, f = _meta(shift)
        assert f('klen_enc', 2).tolist() == [15, 10]                     # min(raw length, T4): SURVEY Q2
        keep = f('keep_enc', 2 * 15).reshape(2, 15)
        assert keep[0].all() and keep[1, :10].all() and not keep[1, 10:].any()
        assert bm['meta'].shape[0] == 2 + 2 + 2 + 2 + 2 * 15 + 3 * 2 * 4 + 2 + 2
        _, f = _meta(shift, T=64, lens=(40, 10), frames=[40])
        assert f('klen_enc', 2).tolist() == [10, 10]
    _meta(None, T=2000, src_max_len=500)
    with pytest.raises(ValueError, match='positional'):
        _meta(None, T=2004, src_max_len=500)


def test_engine_derives_the_shift_from_the_layout():
    from mtl_amd import convstack
    from mtl_amd.engine import ParamLayout
    conv = ParamLayout([('encoder.input_linear.weight', (8, 5120)), ('conv.0.weight', (64, 1, 3, 3))])
    none = ParamLayout([('encoder.input_linear.weight', (8, 161)), ('decoder.output_linear.weight', (4, 8))])
    assert convstack.time_shift(conv) == 2 and convstack.time_shift(none) == 0
    assert convstack.layers_for(conv) is convstack.LAYERS and convstack.layers_for(none) is None


# ---------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import mtl_amd
    lib = mtl_amd._lib.lib()
    p = 4096                                                     # (never dereferenced: every call below returns before a launch)
    ok = dict(B=2, F=161, T=63, N=128)
    fwd = lambda x=p, w=p, y=p, tasks=1, **d: lib.mtl_featproj_fwd_tb(None, x, w, None, y, *[dict(ok, **d)[k] for k in 'BFTN'], tasks, 0, 0, 0)
    need = lib.mtl_featproj_wgrad_workspace(2, 161, 63, 128, 1)
    assert need == 1 * 128 * 161 * 4
    assert lib.mtl_featproj_wgrad_workspace(2, 161, 257, 512, 3) == 3 * 3 * 512 * 161 * 4      # 514 rows: three slices
    wg = lambda x=p, dy=p, dw=p, ws=p, nbytes=need, tasks=1, **d: lib.mtl_featproj_wgrad_tb(
        None, x, dy, dw, ws, nbytes, *[dict(ok, **d)[k] for k in 'BFTN'], tasks, 0, 0, 0)
    for k in 'BFTN':
        for bad in (0, -3):
            assert fwd(**{k: bad}) == -22 and wg(**{k: bad}) == -22 and lib.mtl_featproj_wgrad_workspace(*[dict(ok, **{k: bad})[q] for q in 'BFTN'], 1) == -22
    assert fwd(tasks=0) == -22 and wg(tasks=0) == -22
    for name in ('x', 'w', 'y'):
        assert fwd(**{name: None}) == -22
    for name in ('x', 'dy', 'dw', 'ws'):
        assert wg(**{name: None}) == -22
    assert wg(nbytes=need - 4) == -22 and wg(nbytes=0) == -22


def test_entry_points_are_recordable():
    import mtl_amd
    lib = mtl_amd._lib.lib()
    ops = [lib.mtl_cmdlist_opcode(n.encode()) for n in ('mtl_featproj_fwd_tb', 'mtl_featproj_wgrad_tb')]
    assert all(o >= 0 for o in ops) and ops[0] != ops[1]


# ---------------------------------------------------------------------------------------------------- the bounds of the GPU tests
def _separates(rep, what):
    X.check({'six': rep['six']}, rep['bound'], what)                          # admitted
    assert rep['f32'] < rep['bound'] / 2, (what, rep['f32'], rep['bound'])
    for t, e in rep['drops'].items():
        with pytest.raises(AssertionError):
            X.check({'drop %s' % (t,): e}, rep['bound'], what)


@pytest.mark.parametrize('shape', U.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bounds_separate_six_terms_from_five(shape):
    for t in range(U.TASKS):
        for xt in (t, 0):
            for bias in (True, False):
                _separates(U.fwd_report(shape, t, bias, False, xt), 'fwd %s task %d x %d bias %d' % (shape, t, xt, bias))
            _separates(U.wgrad_report(shape, t, False, xt), 'wgrad %s task %d x %d' % (shape, t, xt))


def test_probe_bounds_separate_six_terms_from_five():
    _separates(U.fwd_report(U.FWD_PROBE, probe=True), 'fwd probe')
    _separates(U.wgrad_report(U.WG_PROBE, probe=True), 'wgrad probe')


# ---------------------------------------------------------------------------------------------------- two parameter groups on several ranks
def _none_layout():
    from mtl_amd.engine import ParamLayout
    return ParamLayout([('encoder.input_linear.weight', (8, 161)), ('encoder.b.bias', (11,)), ('decoder.c.weight', (64, 9)), ('decoder.d.bias', (3,))])


def test_end_of_iteration_all_reduce_posts_decoder_then_encoder_and_nothing_else(monkeypatch):
    """a model without convolutions has no 'conv' group: with chunking on every rank posts the decoder slice, then the encoder slice
    (together the whole buffer); with chunking off the one all-reduce of the whole buffer"""
    import types
    import mtl_amd
    mdist, layout = mtl_amd.dist, _none_layout()
    bounds = layout.group_bounds()
    assert sorted(bounds) == ['decoder', 'encoder'] and bounds['encoder'] == (0, bounds['decoder'][0]) and bounds['decoder'][1] == layout.total
    G = torch.zeros(layout.total)
    posted = []
    monkeypatch.setattr(mdist, 'allreduce_sum_', lambda t: posted.append(((t.data_ptr() - G.data_ptr()) // 4, t.numel())))
    trainer = mtl_amd.TransientTrainer()
    for chunked, want in ((True, [(bounds['decoder'][0], bounds['decoder'][1] - bounds['decoder'][0]), (0, bounds['encoder'][1])]),
                          (False, [(0, layout.total)])):
        monkeypatch.setattr(mdist, 'chunked_on', lambda c=chunked: c)
        del posted[:]
        trainer._G_reduced = False
        trainer.reduce_meta_gradient(types.SimpleNamespace(_G=G, _layout=layout))
        assert posted == want and trainer._G_reduced


def test_chunk_hook_hands_over_decoder_then_encoder_for_a_model_without_convolutions(monkeypatch):
    """metastep._chunk_hook with the collectives and the streams stubbed: the hook the validation backward calls per finished group
    forms and issues exactly that group's slice; a layout with a group of another name is refused"""
    import contextlib
    import types
    import mtl_amd
    from mtl_amd import metastep
    from mtl_amd.engine import ParamLayout
    mdist, layout = mtl_amd.dist, _none_layout()
    bounds = layout.group_bounds()
    G = torch.zeros(layout.total)
    events = []

    class Chunks:
        def issue(self, t):
            events.append(('issue', (t.data_ptr() - G.data_ptr()) // 4, t.numel()))
    stream = types.SimpleNamespace(wait_stream=lambda s: None, cuda_stream=7)
    monkeypatch.setattr(mdist, 'chunked_on', lambda: True)
    monkeypatch.setattr(mdist, 'ChunkedAllReduce', Chunks)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: object())
    monkeypatch.setattr(torch.cuda, 'stream', lambda s: contextlib.nullcontext())
    tr = types.SimpleNamespace(_comm_stream=stream, _chunks=None)
    model = types.SimpleNamespace(_G=G, flat_parameters=G)
    eng = types.SimpleNamespace(slice_bounds=layout.group_bounds, side=None)
    hook = metastep._chunk_hook(tr, model, eng, lambda first, count, raw: events.append(('sum', first, count, raw)))
    for tag in ('decoder', 'encoder'):                       # the order PassEngine.backward hands the groups over in; no third call
        hook(tag)
    d, e = bounds['decoder'], bounds['encoder']
    assert events == [('sum', d[0], d[1] - d[0], 7), ('issue', d[0], d[1] - d[0]), ('sum', e[0], e[1] - e[0], 7), ('issue', e[0], e[1] - e[0])]
    assert d[1] - d[0] + e[1] - e[0] == layout.total
    odd = ParamLayout([('encoder.a', (4,)), ('decoder.b', (4,)), ('other.c', (4,))])
    with pytest.raises(RuntimeError, match='parameter groups'):
        metastep._chunk_hook(tr, model, types.SimpleNamespace(slice_bounds=odd.group_bounds, side=None), lambda *a: None)
