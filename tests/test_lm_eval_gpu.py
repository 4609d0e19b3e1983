"""MI355X: LM evaluation on the device -- the keyed fp64 sums (mtl_nll_key_sum) against numpy fp64, the language-transition keys
(mtl_lm_switch_keys) against a Python restatement, LMEngine.evaluate / evaluate_test against the fp64 restatement tests/gru_ref.py
and against tests/golden/E0.npz (recorded around the reference's real RNNModel), and the training loop with periodic evaluation.

Bounds: keyed sums |sum - ref| <= R 2^-52 sum|row_nll| (the worst case of regrouping an fp64 sum of fp32 terms), counts and keys
exact, evaluation 1e-5 relative on the loss, every window sum and every class sum (what tests/test_lm_rescore_gpu.py and
tests/test_lm_gru_gpu.py hold sequence_nll to).  Largest errors seen: DESIGN.md section 18."""
import argparse
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gru_ref as GR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, EOS = 150, 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ mtl_nll_key_sum
def _key_sum(row, key, seg, nkey):
    """-> (sum (nkey,) f64, count (nkey,) i32) of one mtl_nll_key_sum call; the outputs are pre-filled so that an unwritten entry shows"""
    import mtl_amd
    L = mtl_amd._lib.lib()
    R = row.numel()
    d_row = row.cuda()
    d_key = key.to(torch.int32).cuda() if key is not None else None
    s = torch.full((nkey,), 12345.0, dtype=torch.float64, device='cuda')
    c = torch.full((nkey,), -7, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(L.mtl_nll_key_sum_workspace(R, nkey)) // 8 + 1, dtype=torch.float64, device='cuda')
    rc = L.mtl_nll_key_sum(_stream(), d_row.data_ptr(), d_key.data_ptr() if d_key is not None else None, seg, R, nkey, s.data_ptr(),
                           c.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    assert rc == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), c.cpu().numpy()


def _key_sum_ref(row, key, nkey):
    r, k = row.numpy().astype(np.float64), key.numpy().astype(np.int64)
    ok = (k >= 0) & (k < nkey)
    return np.bincount(k[ok], weights=r[ok], minlength=nkey), np.bincount(k[ok], minlength=nkey)


def _check_key_sum(row, key, seg, nkey, what):
    R = row.numel()
    eff = key if key is not None else torch.arange(R) // seg
    want_s, want_c = _key_sum_ref(row, eff, nkey)
    got_s, got_c = _key_sum(row, key, seg, nkey)
    again_s, again_c = _key_sum(row, key, seg, nkey)
    assert got_s.tobytes() == again_s.tobytes() and got_c.tobytes() == again_c.tobytes(), what       # bit-identical from run to run
    assert got_c.tolist() == want_c.tolist(), what
    nan = np.isnan(want_s)
    assert np.isnan(got_s).tolist() == nan.tolist(), what                                            # a NaN row reaches its own key only
    bound = R * 2.0 ** -52 * float(np.nansum(np.abs(row.numpy().astype(np.float64))))
    err = float(np.max(np.abs(got_s - want_s)[~nan])) if (~nan).any() else 0.0
    print('key_sum %-28s R=%6d nkey=%4d max|err| %.3e bound %.3e' % (what, R, nkey, err, bound))
    assert err <= bound, (what, err, bound)
    assert (got_s[want_c == 0] == 0).all(), what                                                     # an empty key is written as 0


@pytest.mark.parametrize('nkey', [1, 4, 4096])
@pytest.mark.parametrize('R', [1, 256, 257, 70001])
def test_nll_key_sum(R, nkey):
    g = torch.Generator().manual_seed(1000 * nkey + R)
    row = (12.0 * torch.rand(R, generator=g) ** 3).float() + 1e-3
    mixed = torch.randint(-2, nkey + 3, (R,), generator=g)               # keys below 0 and >= nkey are skipped
    if nkey >= 4:
        mixed[mixed == 1] = 2                                            # ... and key 1 stays empty
    _check_key_sum(row, mixed, 1, nkey, 'mixed, skipped and an empty key')
    _check_key_sum(row, torch.full((R,), nkey - 1), 1, nkey, 'all rows on one key')
    _check_key_sum(row, torch.where(torch.arange(R) % 2 == 0, nkey, -1), 1, nkey, 'all rows skipped')
    seg = -(-R // nkey)                                                  # covers every row ...
    while R % seg == 0:
        seg += 1                                                         # ... and the last segment is ragged
    assert (R + seg - 1) // seg <= nkey
    _check_key_sum(row, None, seg, nkey, 'segments, ragged last')
    if R >= 4 * nkey:
        seg = R // (2 * nkey) - 1 if R // (2 * nkey) > 1 else 1          # rows behind segment nkey - 1 are skipped
        _check_key_sum(row, None, seg, nkey, 'segments, tail skipped')
    bad = row.clone()
    bad[R // 2] = float('nan')
    _check_key_sum(bad, mixed.clamp(0, nkey - 1), 1, nkey, 'one NaN row')
    _check_key_sum(bad, None, seg if R < 4 * nkey else -(-R // nkey), nkey, 'one NaN row, segments')


# ---------------------------------------------------------------------------------------------------------- mtl_lm_switch_keys
def _lang_table():
    """ids >= 2: even = a CJK character, odd = a Latin word; 0 <oov> and 1 <eos> are not Chinese"""
    lang = torch.zeros(V, dtype=torch.uint8)
    lang[2::2] = 1
    return lang


def _keys_ref(ids, tgt, lang, eos, nv):
    out = []
    for a, b in zip(ids.tolist(), tgt.tolist()):
        if b < 0 or not (0 <= a < nv) or not (0 <= b < nv) or a == eos or b == eos:
            out.append(-1)
        else:
            out.append((0 if lang[a] else 2) + (0 if lang[b] else 1))
    return out


def test_switch_keys_exact():
    import mtl_amd
    L = mtl_amd._lib.lib()
    lang = _lang_table()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V + 20, (1031,), generator=g)                 # ids >= V among them
    tgt = torch.randint(-1, V + 20, (1031,), generator=g)                # ... and target = -1
    hand = [(2, 4), (2, 3), (3, 2), (3, 5), (EOS, 2), (2, EOS), (EOS, EOS), (0, 2), (2, 0), (2, -1), (V, 2), (2, V), (-1, 2), (V - 1, V - 2)]
    ids[:len(hand)] = torch.tensor([h[0] for h in hand])
    tgt[:len(hand)] = torch.tensor([h[1] for h in hand])
    want = _keys_ref(ids, tgt, lang.tolist(), EOS, V)
    assert want[:len(hand)] == [0, 1, 2, 3, -1, -1, -1, 2, 1, -1, -1, -1, -1, 2]
    assert set(want) == {-1, 0, 1, 2, 3}
    key = torch.full((ids.numel(),), 99, dtype=torch.int32, device='cuda')
    d_ids, d_tgt, d_lang = ids.cuda(), tgt.cuda(), lang.cuda()
    assert L.mtl_lm_switch_keys(_stream(), d_ids.data_ptr(), d_tgt.data_ptr(), d_lang.data_ptr(), EOS, ids.numel(), V, key.data_ptr()) == 0
    assert key.cpu().tolist() == want


# -------------------------------------------------------------------------------------------------------- LMEngine.evaluate
@pytest.fixture(scope='module')
def e0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'E0.npz'))
    return {k: z[k] for k in z.files}


def _perturb(model, spec):
    """tools/make_golden_lm_eval.py `perturb`: the same draws in the same order"""
    g = torch.Generator().manual_seed(spec['noise_seed'])
    with torch.no_grad():
        model.encoder.weight += spec['noise']['enc'] * torch.randn(model.encoder.weight.shape, generator=g)
        if model.decoder.weight is not model.encoder.weight:
            model.decoder.weight += spec['noise']['dec'] * torch.randn(model.decoder.weight.shape, generator=g)
        model.decoder.bias += spec['noise']['bias'] * torch.randn(model.decoder.bias.shape, generator=g)


def _models(kind, H, e0):
    """-> (the product model on the device at the golden record's parameters, its fp64 restatement)"""
    import mtl_amd
    spec = json.loads(bytes(e0['spec']).decode())
    rnn_type, tied = spec['models'][kind]
    torch.manual_seed(spec['seed'])
    model = mtl_amd.lm.RNNModel(rnn_type, V, H, H, spec['nlayers'], spec['dropout'], tie_weights=tied)
    _perturb(model, spec)
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    assert h.hexdigest() == bytes(e0['a/%s_h%d/theta_sha256' % (kind, H)]).decode()     # the very parameters the golden was recorded at
    ref = GR.RNNModel(rnn_type, V, H, H, spec['nlayers'], spec['dropout'], tie_weights=tied)
    ref.load_state_dict(model.state_dict())
    return model.cuda(), ref.double()


def _source(N, B):
    import mtl_amd
    return mtl_amd.lm.batchify(mtl_amd.lm.synth_corpus(5, V, N), B)


def _oracle(ref, source, bptt, lang):
    """the reference's evaluate / evaluate_test loops in fp64 -> (loss, window sums, class sums, class counts, row NLLs (S - 1, B))"""
    S, B = source.shape
    hidden = ref.init_hidden(B)
    wins, rows = [], []
    with torch.no_grad():
        for i in range(0, S - 1, bptt):
            T = min(bptt, S - 1 - i)
            out, hidden = ref(source[i:i + T], hidden)
            nll = F.cross_entropy(out.view(T * B, -1), source[i + 1:i + 1 + T].reshape(-1), reduction='none')
            wins.append(float(nll.sum()))
            rows.append(nll.view(T, B))
    rows = torch.cat(rows)
    loss = sum(w / B for w in wins) / S                                  # sum_w T_w mean_w / len(data_source)
    keys = _keys_ref(source[:-1].reshape(-1), source[1:].reshape(-1), lang.tolist(), EOS, V)
    cs, cc = [0.0] * 4, [0] * 4
    for k, v in zip(keys, rows.reshape(-1).tolist()):
        if k >= 0:
            cs[k] += v
            cc[k] += 1
    return loss, np.array(wins), np.array(cs), cc, rows


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.abs(np.asarray(b, dtype=np.float64))))


STREAMS = [(70, 3, 5), (41, 1, 5), (330, 10, 7)]


@pytest.mark.parametrize('N,B,bptt', STREAMS)
@pytest.mark.parametrize('H', [32, 128])
@pytest.mark.parametrize('kind', ['lstm', 'gru', 'lstm_tied'])
def test_evaluate_matches_restatement_and_golden(kind, H, N, B, bptt, e0):
    model, ref = _models(kind, H, e0)
    eng = model.engine
    persistent = bool(eng.lib.mtl_gru_layer_supported(B, H) if kind == 'gru' else eng.lib.mtl_lstm_layer_supported(B, H))
    assert persistent == (H == 128) and eng.persistent                  # H = 32 takes the per-step path
    model.train()                                                        # evaluation mode whatever model.training says
    source, lang = _source(N, B), _lang_table()
    S = source.shape[0]
    W = (S - 1 + bptt - 1) // bptt
    assert (S - 1) % bptt == {70: 2, 41: 0, 330: 4}[N]                   # ragged last windows of 2 and 4 steps
    loss, wins, cs, cc, rows = _oracle(ref, source, bptt, lang)
    assert min(cc) > 0, cc                                               # every transition class is populated
    if (N, B, bptt) == (70, 3, 5):
        assert cc == [19, 13, 13, 19] and (S - 1) * B - sum(cc) == 2
    theta, d_src, d_lang = model.flat_parameters, source.cuda(), lang.cuda()
    seed_state = torch.cuda.get_rng_state()
    got = {cw: eng.evaluate(theta, d_src, bptt, lang=d_lang, eos_id=EOS, chunk_windows=cw, rows=True) for cw in (1, 2, None)}
    assert torch.equal(torch.cuda.get_rng_state(), seed_state) and model.training       # no random number drawn, mode untouched
    worst = 0.0
    for cw, res in got.items():
        assert isinstance(res['loss'], float) and res['window_sum'].shape == (W,) and res['window_sum'].dtype == np.float64
        assert res['class_sum'].shape == (4,) and res['class_count'].tolist() == cc
        errs = (_rel(res['loss'], loss), _rel(res['window_sum'], wins), _rel(res['class_sum'], cs))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-5, (cw, errs)
        assert tuple(res['row_logp'].shape) == (S - 1, B) and res['row_logp'].dtype == torch.float32
        # rows: fp32 log-sum-exp minus an fp32 logit, each of magnitude <= max NLL: 1e-5 of the largest row
        assert float((res['row_logp'].cpu().double() + rows).abs().max()) <= 1e-5 * float(rows.max())
    for cw in (1, 2):                                                    # chunkings agree with each other within the same bound
        assert _rel(got[cw]['loss'], got[None]['loss']) <= 1e-5 and _rel(got[cw]['window_sum'], got[None]['window_sum']) <= 1e-5
        assert _rel(got[cw]['class_sum'], got[None]['class_sum']) <= 1e-5
    # tests/golden/E0.npz (a): the loop around the reference's real RNNModel; its windows are len(data) * mean = window_sum / B
    pre = 'a/%s_h%d/n%d/' % (kind, H, N)
    g_err = max(_rel(got[None]['loss'], e0[pre + 'loss']), _rel(got[None]['window_sum'] / B, e0[pre + 'window_loss']))
    assert e0[pre + 'window_loss'].shape == (W,) and g_err <= 1e-5, g_err
    print('evaluate %-9s H=%3d N=%3d B=%2d: worst relative error %.3e (restatement), %.3e (golden)' % (kind, H, N, B, worst, g_err))
    # without lang / rows: nothing of either is returned, the loss is the same
    plain = eng.evaluate(theta, d_src, bptt)
    assert plain['class_sum'] is None and plain['class_count'] is None and 'row_logp' not in plain
    assert plain['loss'] == got[None]['loss']
    # row_logp = -row_nll of a direct mtl_lm_nll_fwd call on the same rows (one recurrent call over the whole stream)
    R = (S - 1) * B
    zero = torch.zeros(model.nlayers, B, H, device='cuda')
    rec = eng._recurrent(theta, d_src[:-1], zero if kind == 'gru' else (zero, zero), 0.0)
    row = torch.empty(R, device='cuda')
    ws = torch.empty(int(eng.lib.mtl_lm_nll_workspace(R, V)) // 4 + 1, device='cuda')
    tgt = d_src[1:].reshape(-1).contiguous()
    P = theta.data_ptr()
    assert eng.lib.mtl_lm_nll_fwd(_stream(), rec['last'].data_ptr(), H, P + 4 * eng.off('decoder.weight'), P + 4 * eng.off('decoder.bias'),
                                  tgt.data_ptr(), R, H, V, B, row.data_ptr(), None, ws.data_ptr(), ws.numel() * 4) == 0
    eng.check_handoff()
    assert torch.equal(got[None]['row_logp'].reshape(-1), -row)


@pytest.mark.parametrize('kind,H', [('lstm', 128), ('gru', 32), ('lstm_tied', 32)])
def test_training_step_after_an_evaluation_is_unchanged(kind, H, e0):
    model, _ = _models(kind, H, e0)
    model.train()
    eng, theta = model.engine, model.flat_parameters
    g = torch.Generator().manual_seed(4)
    x, y = torch.randint(0, V, (6, 4), generator=g).cuda(), torch.randint(0, V, (24,), generator=g).cuda()
    h0 = model.init_hidden(4)

    def step():
        torch.manual_seed(77)
        out = eng.forward(theta, x, y, h0, 0.2)
        grad = torch.zeros_like(theta)
        eng.backward(grad, 1.0)
        eng.check_handoff()
        return float(out['loss']), grad
    loss_a, grad_a = step()
    eng.forward(theta, x, y, h0, 0.2)
    eng.evaluate(theta, _source(70, 3).cuda(), 5, lang=_lang_table().cuda(), eos_id=EOS)
    with pytest.raises(RuntimeError, match='backward'):                  # the evaluation invalidated the pending backward
        eng.backward(torch.zeros_like(theta), 1.0)
    loss_b, grad_b = step()
    assert loss_a == loss_b and torch.equal(grad_a, grad_b) and float(grad_a.abs().sum()) > 0


def _dictionary():
    import mtl_amd
    d = mtl_amd.lm.Dictionary()
    for w in ['<oov>', '<eos>'] + [chr(0x4e00 + i) if i % 2 == 0 else 'w%03d' % i for i in range(2, V)]:
        d.add_word(w)
    return d


def test_evaluate_test_tuple_order_and_empty_classes(e0):
    import mtl_amd
    model, ref = _models('lstm', 32, e0)
    d = _dictionary()
    assert mtl_amd.lm.language_table(d, V, 'cpu').tolist() == _lang_table().tolist()
    source = _source(70, 3)
    loss, wins, cs, cc, _ = _oracle(ref, source, 5, _lang_table())
    out = mtl_amd.lm.evaluate_test(model, source.cuda(), d, bptt=5)
    want = (loss, cs[0] / cc[0], cs[1] / cc[1], cs[2] / cc[2], cs[3] / cc[3], (cs[1] + cs[2]) / (cc[1] + cc[2]))
    assert isinstance(out, tuple) and len(out) == 6 and all(isinstance(v, float) for v in out)
    assert len({round(v, 6) for v in want}) == 6                        # six different numbers: a permutation would show
    assert max(abs(a - b) / abs(b) for a, b in zip(out, want)) <= 1e-5
    assert mtl_amd.lm.evaluate(model, source, bptt=5) == out[0]
    # an all-Chinese stream: only zh->zh is populated, the other means are nan (the reference would raise ZeroDivisionError)
    zh = torch.tensor([2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28], dtype=torch.int64).view(7, 2).cuda()
    out = mtl_amd.lm.evaluate_test(model, zh, d, bptt=4)
    assert math.isfinite(out[0]) and math.isfinite(out[1]) and all(math.isnan(v) for v in out[2:])


# ---------------------------------------------------------------------------------------------------------------- the loop
def _loop_setup(corpora, seed=21):
    import mtl_amd
    torch.manual_seed(seed)
    model = mtl_amd.lm.RNNModel('LSTM', V, 32, 32, 2, 0.2).cuda()
    ds = mtl_amd.lm.LMDataset(corpora, argparse.Namespace(bptt=5, batch_size=4, cuda=False))
    tr = mtl_amd.lm.LMMetaTrainer(model, lr=2.0, meta_lr_factor=3.0, clip=0.25, ratio=0.8)
    torch.manual_seed(seed + 1)                                          # the keep-mask seeds of the run
    return model, ds, tr


def test_train_with_periodic_evaluation(tmp_path, capsys):
    import mtl_amd
    lm = mtl_amd.lm
    corpora = [lm.synth_corpus(s, V, 203) for s in (1, 2)]
    val, test = lm.batchify(lm.synth_corpus(9, V, 203), 4).cuda(), lm.batchify(lm.synth_corpus(10, V, 123), 4).cuda()
    d, path = _dictionary(), str(tmp_path / 'best.pt')
    model_a, ds, tr = _loop_setup(corpora)
    out = tr.train(ds, 0, 3, valid_interval=2, val_data=val, test_data=test, save_path=path, dictionary=d)
    printed = capsys.readouterr().out
    model_b, ds, tr_b = _loop_setup(corpora)
    assert tr_b.train(ds, 0, 3) is None
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)                 # the evaluation changed nothing the training reads
    assert model_a.training and tr.lr == 2.0
    for a, b in zip(tr.hidden, tr_b.hidden):
        assert torch.equal(a, b)
    v, t = lm.evaluate(model_a, val, 5), lm.evaluate(model_a, test, 5)
    assert out == dict(best_val_loss=v, evaluations=[(2, v, t, 2.0)], stopped_early=False)
    assert 'it 2 | val loss {:5f} | ppl {:5f}'.format(v, math.exp(v)) in printed and 'it 2 | test loss {:5f}'.format(t) in printed
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert ck['tie_weights'] is False and ck['rnn_type'] == 'LSTM'
    for k, p in model_a.state_dict().items():
        assert torch.equal(ck['model_state_dict'][k], p.cpu()), k
    # the saved file rescoring a string = sequence_nll on the live model
    scorer = mtl_amd.LM(path)
    s = 'w003 %s w005 nope %s' % (chr(0x4e00 + 4), chr(0x4e00 + 6))
    ids, oov = scorer.seq_to_tensor(s)
    assert oov == 1
    live = float(model_a.engine.sequence_nll(model_a.flat_parameters, ids[:-1].view(-1, 1).cuda(), ids[1:].view(-1, 1).cuda())[0])
    got = float(scorer.evaluate(s)[0])
    assert abs(got - live) <= 1e-6 * abs(live)                          # LM.score's fp32 n * (nll / n)


def test_train_anneals_and_stops_early():
    """the tasks teach 'token 5 follows token 5'; the validation stream is all token 7, so its loss rises with every step"""
    import mtl_amd
    lm = mtl_amd.lm
    model, ds, tr = _loop_setup([torch.full((203,), 5, dtype=torch.int64)] * 2)
    val = lm.batchify(torch.full((83,), 7, dtype=torch.int64), 4).cuda()
    out = tr.train(ds, 0, 20, valid_interval=1, val_data=val, patience=2)
    ev = out['evaluations']
    assert [e[0] for e in ev] == [1, 2, 3] and out['stopped_early'] and out['best_val_loss'] == ev[0][1]
    assert ev[0][1] < ev[1][1] < ev[2][1] and all(e[2] is None for e in ev)
    assert [e[3] for e in ev] == [2.0, 0.5, 0.125] and tr.lr == 0.125
