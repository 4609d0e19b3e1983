"""MI355X: the fused LM NLL kernel (mtl_lm_nll_fwd) against torch fp64 and against the gemm + cross-entropy pair, LM.evaluate /
calculate_lm_score against the reference's recorded values, and Transformer.evaluate(beam_search=True, lm_rescoring=True) against
the reference's rescored n-best lists (tests/golden/R0.npz)."""
import argparse

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import lm_rescore_util as lu

pytestmark = pytest.mark.gpu


def _nll_case(T, B, H, V, seed, ragged=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(T * B, H, generator=g))
    W = 0.15 * torch.randn(V, H, generator=g)
    b = 0.5 * torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (T, B), generator=g)
    if ragged:
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0] = T
        tgt[torch.arange(T).unsqueeze(1) >= lens.unsqueeze(0)] = -1
    return x, W, b, tgt.reshape(-1)


def _run_nll(L, x, W, b, tgt, B):
    R, H = x.shape
    V = W.shape[0]
    dx, dW, db, dt = x.cuda(), W.cuda(), b.cuda(), tgt.cuda()
    row, seq = torch.full((R,), 7.0, device='cuda'), torch.full((B,), 7.0, device='cuda')
    ws = torch.empty(int(L.mtl_lm_nll_workspace(R, V)) // 4 + 1, device='cuda')
    rc = L.mtl_lm_nll_fwd(torch.cuda.current_stream().cuda_stream, dx.data_ptr(), H, dW.data_ptr(), db.data_ptr(), dt.data_ptr(), R, H, V, B,
                          row.data_ptr(), seq.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    assert rc == 0
    torch.cuda.synchronize()
    return row.cpu(), seq.cpu()


@pytest.mark.parametrize('T,B,H,V', [(5, 3, 32, 150), (9, 29, 200, 30011), (4, 67, 650, 30011), (3, 1, 650, 150), (7, 5, 200, 150)])
def test_lm_nll_matches_fp64(T, B, H, V):
    import mtl_amd
    L = mtl_amd._lib.lib()
    x, W, b, tgt = _nll_case(T, B, H, V, seed=T * 1000 + H)
    row, seq = _run_nll(L, x, W, b, tgt, B)
    logits = x.double() @ W.double().t() + b.double()
    valid = tgt >= 0
    ref = torch.zeros(T * B, dtype=torch.float64)
    ref[valid] = torch.logsumexp(logits[valid], 1) - logits[valid].gather(1, tgt[valid].unsqueeze(1)).squeeze(1)
    assert torch.all(row[~valid] == 0)
    err = ((row.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    assert err <= 1e-5, err
    ref_seq = ref.view(T, B).sum(0)
    err = ((seq.double() - ref_seq).abs() / ref_seq.abs().clamp_min(1.0)).max().item()
    assert err <= 1e-5, err
    row2, seq2 = _run_nll(L, x, W, b, tgt, B)                     # no atomics: bit-identical
    assert torch.equal(row, row2) and torch.equal(seq, seq2)


def test_lm_nll_agrees_with_gemm_and_cross_entropy():
    """the existing two-step path (logits by mtl_gemm_f32_ex, then mtl_ce_argmax_fwd) on the valid rows"""
    import mtl_amd
    L = mtl_amd._lib.lib()
    T, B, H, V = 8, 32, 200, 30011
    x, W, b, tgt = _nll_case(T, B, H, V, seed=3)
    row, _ = _run_nll(L, x, W, b, tgt, B)
    R, st = T * B, torch.cuda.current_stream().cuda_stream
    dx, dW, db, dt = x.cuda(), W.cuda(), b.cuda(), tgt.cuda()
    logits = torch.empty(R, V, device='cuda')
    ws = torch.empty(4 << 20, device='cuda')
    assert L.mtl_gemm_f32_ex(st, 0, 1, R, V, H, 1.0, dx.data_ptr(), H, dW.data_ptr(), H, logits.data_ptr(), V, db.data_ptr(), None, 0, 0, 1, 1,
                             0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0) == 0
    lse, hyp, rowloss, loss = (torch.empty(R, device='cuda'), torch.empty(R, dtype=torch.int64, device='cuda'), torch.empty(R, device='cuda'),
                               torch.empty(1, device='cuda'))
    assert L.mtl_ce_argmax_fwd(st, logits.data_ptr(), dt.data_ptr(), R, V, V, -1, 0.0, R, None, lse.data_ptr(), hyp.data_ptr(),
                               rowloss.data_ptr(), loss.data_ptr()) == 0
    valid = tgt >= 0
    pair = (lse.cpu() - logits.cpu().gather(1, tgt.clamp_min(0).unsqueeze(1)).squeeze(1))[valid]
    err = ((row[valid] - pair).abs() / pair.abs().clamp_min(1.0)).max().item()
    assert err <= 1e-5, err


@pytest.fixture(scope='module')
def r0():
    return lu.load_r0()


@pytest.fixture(scope='module')
def r0_lm(r0, tmp_path_factory):
    import mtl_amd
    path, _ = lu.r0_checkpoint(r0, str(tmp_path_factory.mktemp('lm') / 'lm.pt'))
    return mtl_amd.LM(path, argparse.Namespace(cuda=True))


def test_lm_evaluate_and_calculate_lm_score_match_the_reference(r0, r0_lm):
    import mtl_amd
    vocab = lu.r0_vocab(r0)
    assert r0_lm.model.flat_parameters.is_cuda
    for yseq, sc, nw, oov in zip(r0['hand_ids'], r0['hand_score'], r0['hand_num_words'], r0['hand_oov']):
        got = mtl_amd.calculate_lm_score(torch.tensor([yseq]), r0_lm, vocab)
        if nw == 0:
            assert got == (-999, 0, 0)
            continue
        assert (got[1], got[2]) == (int(nw), int(oov))
        assert abs(float(got[0]) - float(sc)) <= 1e-5 * abs(float(sc)), (float(got[0]), float(sc))
        assert mtl_amd.calculate_lm_score(list(yseq), r0_lm, vocab)[0] == got[0]
    # batched scoring == one string at a time (batch of 1: the persistent LSTM stack; batch of all: the per-step path)
    total, oovs = r0_lm.score(r0['lm_seen'])
    for s, t, o in zip(r0['lm_seen'][:8], total, oovs):
        one, o1 = r0_lm.evaluate(s)
        assert o1 == o and abs(float(one) - float(t)) <= 1e-5 * abs(float(t))


def _r0_model(r0):
    import mtl_amd
    from oracle import refimpl as R
    z, cfg, spec = gu.load('F0')
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
                              emb_trg_sharing=False, label_smoothing=0.0, name='r0', lr=spec['lr'], meta_lr=spec['meta_lr'],
                              k_train=spec['k'], k_valid=spec['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_ckpt',
                              cuda=True, **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    vocab = lu.r0_vocab(r0)
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    gu.perturb_output_layer(model.decoder.output_linear.weight, r0['spec'])
    model = model.cuda()
    s = r0['spec']
    args.beam_width, args.beam_nbest, args.tgt_max_len = s['beam_width'], s['nbest'], cfg['tgt_max_len']
    x, lens, y = R.synth_batch(s['seed'], s['k'], s['T'], s['L'], cfg['vocab_size'], True)
    return model, args, vocab, (x, lens, y)


def _expected(r0):
    """the reference's n-best ids and final scores per utterance"""
    out, i = [], 0
    for n in r0['ended_count']:
        k = min(n, r0['spec']['nbest'])
        out.append((r0['ended_ids'][i:i + k], r0['ended_final'][i:i + k]))
        i += n
    return out


def test_beam_search_with_lm_rescoring_matches_the_reference(r0, r0_lm):
    import mtl_amd
    model, args, vocab, (x, lens, y) = _r0_model(r0)
    s = r0['spec']
    kw = dict(beam_search=True, lm_rescoring=True, lm=r0_lm, lm_weight=s['lm_weight'], c_weight=s['c_weight'], start_token=vocab.SOS_ID)
    _, hyps, _ = model.evaluate(x.cuda(), lens, y, args, **kw)
    assert model.last_beam_ids == r0['lm_ids']
    assert hyps == r0['lm_strs']
    exp = _expected(r0)
    assert [q for ids, _ in exp for q in ids] == r0['lm_ids']
    ref_final = np.concatenate([f for _, f in exp]).astype(np.float64)
    got = np.array(model.last_beam_scores, dtype=np.float64)
    assert np.max(np.abs(got - ref_final) / np.abs(ref_final)) <= 1e-5
    assert r0['lm_ids'] != r0['plain_ids']               # the LM changed the order
    # the 52 ended hypotheses of the batch run through the per-step LSTM (B > 32); the first three utterances (<= 32 hypotheses)
    # through the persistent stack: same rankings
    L = mtl_amd._lib.lib()
    nh = sum(r0['ended_count'])
    assert nh > 32 and not L.mtl_lstm_stack_supported(nh, s['lm_nhid'], s['lm_nlayers'])
    assert sum(r0['ended_count'][:3]) <= 32 and L.mtl_lstm_stack_supported(sum(r0['ended_count'][:3]), s['lm_nhid'], s['lm_nlayers'])
    _, hyps3, _ = model.evaluate(x[:3].cuda(), lens[:3], y[:3], args, **kw)
    n3 = sum(len(ids) for ids, _ in exp[:3])
    assert model.last_beam_ids == r0['lm_ids'][:n3] and hyps3 == r0['lm_strs'][:n3]
    got3 = np.array(model.last_beam_scores, dtype=np.float64)
    assert np.max(np.abs(got3 - ref_final[:n3]) / np.abs(ref_final[:n3])) <= 1e-5
    # the default call is untouched by an LM argument when rescoring is off, and the greedy search ignores lm_rescoring
    _, plain, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=True, lm=r0_lm, start_token=vocab.SOS_ID)
    assert model.last_beam_ids == r0['plain_ids']
    _, g1, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=False, lm_rescoring=True, lm=r0_lm, start_token=vocab.SOS_ID,
                               max_steps=50)
    _, g2, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=False, start_token=vocab.SOS_ID, max_steps=50)
    assert g1 == g2


def test_sequence_nll_paths_agree_and_leave_training_intact(r0, r0_lm):
    """LMEngine.sequence_nll: persistent stack vs per-step LSTM on the same ragged batch, and against RNNModel.forward's logits"""
    import mtl_amd
    eng = r0_lm.model.engine
    g = torch.Generator().manual_seed(1)
    T, B, V = 6, 20, r0['spec']['lm_ntoken']
    ids = torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T, B), generator=g)
    tgt[4:, ::3] = -1
    a = eng.sequence_nll(r0_lm.model.flat_parameters, ids, tgt).cpu()
    eng.persistent = False
    try:
        b = eng.sequence_nll(r0_lm.model.flat_parameters, ids, tgt).cpu()
    finally:
        eng.persistent = True
    assert torch.allclose(a, b, rtol=1e-5, atol=0)
    with pytest.raises(RuntimeError, match='backward'):
        eng.backward(torch.zeros_like(r0_lm.model.flat_parameters))        # sequence_nll reused forward()'s buffers
    logits, _ = r0_lm.model(ids.cuda(), r0_lm.model.init_hidden(B))
    lp = torch.log_softmax(logits.double().cpu(), -1)
    ref = -(lp.gather(2, tgt.clamp_min(0).unsqueeze(2)).squeeze(2) * (tgt >= 0)).sum(0)
    assert torch.allclose(a.double(), ref, rtol=1e-5, atol=0)
    assert isinstance(r0_lm.model, mtl_amd.lm.RNNModel) and not r0_lm.model.training
