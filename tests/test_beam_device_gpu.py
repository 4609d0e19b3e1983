"""MI355X: the device-resident beam search -- mtl_beam_rank against a numpy restatement of one position (bit for bit), mtl_beam_gather
against index_select, PassEngine.beam_decode_batch against the host-ranked beam_decode (exact), Transformer.evaluate(device_ranking=True)
against the reference's goldens (B0, R0) and the CPU oracle, and evaluate_test_set against the reference's recorded test-set
evaluation (tests/golden/T0.npz)."""
import argparse
import contextlib
import io
import re

import numpy as np
import pytest
import torch

from tests import beam_util as bu
from tests import eval_util as tu
from tests import golden_util as gu
from tests import lm_rescore_util as lu

pytestmark = pytest.mark.gpu


def _lib():
    import mtl_amd
    return mtl_amd._lib.lib()


def _rank_on_device(state, logits, lse, tok, parent, i, T4, U, W, V, S, eos):
    d_state, d_logits, d_lse = torch.from_numpy(state).cuda(), torch.from_numpy(logits).cuda(), torch.from_numpy(lse).cuda()
    d_tok, d_par = torch.from_numpy(tok).cuda(), torch.from_numpy(parent).cuda()
    rc = _lib().mtl_beam_rank(torch.cuda.current_stream().cuda_stream, d_logits.data_ptr(), d_lse.data_ptr(), d_state.data_ptr(),
                              d_tok.data_ptr(), d_par.data_ptr(), i, T4, U, W, V, S, eos)
    assert rc == 0
    torch.cuda.synchronize()
    return d_state.cpu().numpy(), d_tok.cpu().numpy(), d_par.cpu().numpy()


@pytest.mark.parametrize('W', [1, 3, 5])
@pytest.mark.parametrize('V', [97, 3765])
def test_rank_kernel_matches_the_numpy_restatement_bit_for_bit(W, V):
    """one position for every live count n = 1..W: utterance 0 on random logits and scores, utterance 1 already done (must stay
    untouched), utterance 2 with equal scores on equal rows and equal values inside a row (the tie rule), utterance 3 with EOS among
    the best entries of its rows (emitted EOS); at an inner position and at the forced-EOS position T4 - 1"""
    U, S, T4, eos = 4, 9, 7, 2
    rng = np.random.RandomState(100 * W + V)
    for n in range(1, W + 1):
        for i in (3, T4 - 1):
            logits = rng.randn(U * W, V).astype(np.float32)
            for r in range(W):                                          # utterance 2: every row the same, two equal maxima per row
                logits[2 * W + r] = logits[2 * W]
            logits[2 * W:3 * W, 11] = logits[2 * W:3 * W, 60] = np.float32(5.0)
            logits[3 * W:4 * W, eos] = np.float32(6.0)                  # utterance 3: EOS is the best entry of every row
            if W > 1:
                logits[3 * W + 1, eos] = np.float32(-4.0)               # ... but not of row 1
            lse = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
            scores = rng.randn(U, W).astype(np.float32) - 3
            scores[2, :] = np.float32(-1.25)
            scores[3, :] = np.float32(-2.0)
            state = bu.new_state(U, W, S, [n, max(1, n - 1), n, n], scores, done=[0, 1, 0, 0], ended=[2, 1, 0, 3])
            tok = np.full(U * W, 77, dtype=np.int64)
            par = np.full(U * W, -3, dtype=np.int32)
            exp_state, exp_tok, exp_par = state.copy(), tok.copy(), par.copy()
            bu.rank_position(exp_state, logits, lse, exp_tok, exp_par, i, T4, U, W, V, S, eos)
            got_state, got_tok, got_par = _rank_on_device(state, logits, lse, tok, par, i, T4, U, W, V, S, eos)
            what = 'W=%d V=%d n=%d i=%d' % (W, V, n, i)
            assert np.array_equal(got_state, exp_state), what                # integers and fp32 bit patterns alike
            assert np.array_equal(got_tok, exp_tok) and np.array_equal(got_par, exp_par), what
            # what the cases are there for
            o_score, o_bp, o_tk, o_en, _ = bu.state_offsets(U, W, S)
            assert np.array_equal(got_state[4:8], state[4:8]) and np.all(got_tok[W:2 * W] == 77) and np.all(got_par[W:2 * W] == -3)
            if i == T4 - 1:
                assert all(got_state[4 * u + 1] == 1 and got_state[4 * u] == 0 for u in (0, 2, 3))
                assert got_state[2] == 2 + W and got_state[o_en + 5 * 2 + 4] == 1        # forced entries behind the two old ones
            else:
                # ties: all candidates of utterance 2's rows 0.. are equal pairwise -> row 0's best two ids, lower id first
                if W >= 2:
                    assert got_tok[2 * W] == 11 and got_tok[2 * W + 1] == 60 and got_par[2 * W] == got_par[2 * W + 1] == 2 * W
                # emitted EOS: utterance 3's best candidate is row 0's EOS -> a new ended entry that is not a forced one
                assert got_state[4 * 3 + 2] > 3 and got_state[o_en + 5 * (3 * S * W + 3) + 3] == eos and got_state[o_en + 5 * (3 * S * W + 3) + 4] == 0


def test_gather_matches_index_select():
    L = _lib()
    rows, S, width, t = 15, 12, 128, 5
    g = torch.Generator().manual_seed(4)
    for parent in ([0, 0, 2, 1, 4, 3, 3, 7, 8, 5, 10, 11, 14, 13, 12], list(range(rows)), [14 - r for r in range(rows)]):
        caches = [torch.randn(rows, S, width, generator=g).cuda() for _ in range(4)]
        orig = [c.clone() for c in caches]
        tab = torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64).cuda()
        par = torch.tensor(parent, dtype=torch.int32).cuda()
        tmp = torch.empty(4 * rows * t * width).cuda()
        rc = L.mtl_beam_gather(torch.cuda.current_stream().cuda_stream, tab.data_ptr(), 4, par.data_ptr(), tmp.data_ptr(), tmp.numel(), rows, t,
                               width, S * width)
        assert rc == 0
        torch.cuda.synchronize()
        idx = torch.tensor(parent, dtype=torch.int64).cuda()
        for c, o in zip(caches, orig):
            assert torch.equal(c[:, :t], o.index_select(0, idx)[:, :t]) and torch.equal(c[:, t:], o[:, t:])


def _f0_model(perturb_spec):
    import mtl_amd
    z, cfg, spec = gu.load('F0')
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
                              dropout=0.0, emb_trg_sharing=False, label_smoothing=0.0, name='beamdev', lr=spec['lr'],
                              meta_lr=spec['meta_lr'], k_train=spec['k'], k_valid=spec['k'], clip=False, max_norm=400,
                              save_every=10 ** 9, save_folder='/tmp/mtl_ckpt', cuda=True,
                              **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    vocab = mtl_amd.synthetic_vocab(cfg['vocab_size'])
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    gu.perturb_output_layer(model.decoder.output_linear.weight, perturb_spec)
    return model.cuda(), args, vocab, cfg


def _memory(model, x, lens, y):
    """the encoder output of the batch as Transformer.evaluate hands it to the searches -> (tensor (B, T4, d), T4)"""
    eng = model.engine
    model.eval()
    widen, eng.widen = eng.widen, '0'
    try:
        model.pass_forward(x.cuda(), lens, y)
    finally:
        eng.widen = widen
    mem = eng.arena['e%d.ff.y' % (eng.hp.n_enc - 1)].clone()
    return mem, (x.shape[3] // 2) // 2


# (seed, utterances, frames, labels, W, nbest, tgt_max_len)
EXACT_CASES = [(11, 3, 64, 6, 5, 3, 100), (12, 4, 80, 5, 3, 1, 100), (13, 2, 72, 8, 1, 1, 100), (14, 3, 96, 6, 5, 1, 100),
               (15, 3, 64, 6, 3, 3, 10), (16, 2, 48, 4, 5, 3, 100)]


@pytest.mark.parametrize('seed,k,T,L,W,nbest,tgt', EXACT_CASES)
def test_device_ranked_search_equals_the_host_ranked_search(seed, k, T, L, W, nbest, tgt):
    """same engine, one utterance per session: ids, fp32 scores, order and the ended lists are EQUAL -- the logits are the same, so the
    decisions must be; three rounds (eager, recording, replay of the command lists)"""
    from oracle import refimpl as R
    bspec = gu.load_beam()[0]
    model, args, vocab, cfg = _f0_model(bspec)
    eng = model.engine
    x, lens, y = R.synth_batch(seed, k, T, L, cfg['vocab_size'], True)
    mem, T4 = _memory(model, x, lens, y)
    assert (tgt < T4) == (tgt == 10)
    nw = model._num_words
    theta = model.flat_parameters
    for rnd in range(3):
        host, host_ended = [], []
        for b in range(k):
            e = []
            host.append(eng.beam_decode(theta, mem.data_ptr() + 4 * b * T4 * eng.hp.d, T4, vocab.SOS_ID, W, nbest, tgt, nw, vocab.EOS_ID, 1.0,
                                        ended_out=e))
            host_ended.append(e)
        dev_ended = [[] for _ in range(k)]
        dev = eng.beam_decode_batch(theta, mem.data_ptr(), k, T4, vocab.SOS_ID, W, nbest, tgt, nw, vocab.EOS_ID, 1.0, ended_out=dev_ended,
                                    chunk=1)
        assert dev == host, (rnd, dev, host)
        assert len(dev_ended) == len(host_ended)
        for a, b_ in zip(dev_ended, host_ended):
            assert [h['yseq'] for h in a] == [h['yseq'] for h in b_], rnd
            assert [np.float32(h['score']).tobytes() for h in a] == [np.float32(h['score']).tobytes() for h in b_], rnd
        if tgt >= T4:
            assert all(len(r) >= 1 for r in host)
    assert eng.replay_beam_batch.recorded()                                  # the blocks of positions were recorded and replayed


@contextlib.contextmanager
def _chunk_of(model, U):
    eng = model.engine
    if U is None:
        yield
        return
    eng.beam_chunk = lambda W: U
    try:
        yield
    finally:
        del eng.beam_chunk


@pytest.mark.parametrize('U', [None, 1])
def test_reference_goldens_through_device_ranking(U, tmp_path):
    """B0's ids and strings, R0's plain and LM-rescored n-best lists with their scores, through evaluate(device_ranking=True): with the
    chunk size the engine picks (several utterances per decoder step) and with one utterance per session"""
    import mtl_amd
    from oracle import refimpl as R
    bspec, ids, strs, eval_strs = gu.load_beam()
    model, args, vocab, cfg = _f0_model(bspec)
    args.beam_width, args.beam_nbest, args.tgt_max_len = bspec['beam_width'], bspec['nbest'], cfg['tgt_max_len']
    x, lens, y = R.synth_batch(bspec['seed'], bspec['k'], bspec['T'], bspec['L'], cfg['vocab_size'], True)
    if U is None:
        assert model.engine.beam_chunk(bspec['beam_width']) > 1
    with _chunk_of(model, U):
        _, hyps, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=vocab.SOS_ID, device_ranking=True)
    assert model.last_beam_ids == ids
    assert hyps == strs == eval_strs

    r0 = lu.load_r0()
    s = r0['spec']
    path, _ = lu.r0_checkpoint(r0, str(tmp_path / 'lm.pt'))
    lm = mtl_amd.LM(path, argparse.Namespace(cuda=True))
    vocab = lu.r0_vocab(r0)
    model = tu.t0_model(mtl_amd, vocab, tgt_max_len=cfg['tgt_max_len']).cuda()
    args = argparse.Namespace(beam_width=s['beam_width'], beam_nbest=s['nbest'], tgt_max_len=cfg['tgt_max_len'])
    x, lens, y = R.synth_batch(s['seed'], s['k'], s['T'], s['L'], cfg['vocab_size'], True)
    with _chunk_of(model, U):
        _, plain, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=True, lm=lm, start_token=vocab.SOS_ID, device_ranking=True)
        assert model.last_beam_ids == r0['plain_ids']
        _, hyps, _ = model.evaluate(x.cuda(), lens, y, args, beam_search=True, lm_rescoring=True, lm=lm, lm_weight=s['lm_weight'],
                                    c_weight=s['c_weight'], start_token=vocab.SOS_ID, device_ranking=True)
    assert model.last_beam_ids == r0['lm_ids']
    assert hyps == r0['lm_strs']
    ref_final, i = [], 0
    for n in r0['ended_count']:
        ref_final.extend(r0['ended_final'][i:i + min(n, s['nbest'])])
        i += n
    ref_final = np.array(ref_final, dtype=np.float64)
    got = np.array(model.last_beam_scores, dtype=np.float64)
    assert np.max(np.abs(got - ref_final) / np.abs(ref_final)) <= 1e-5          # (the tolerance of tests/test_lm_rescore_gpu.py)


# (seed, utterances, frames, labels, W, nbest) and the batch's smallest decision margin on the CPU oracle (tests/beam_util.py
# oracle_beam_margin: the gap between the W-th and the (W + 1)-th candidate score at any position).  The seeds were chosen on the CPU
# for margins >= 1e-3 -- about two orders above the 1.3e-5 worst device-vs-oracle error the project records -- so that the decisions do
# not hinge on rounding: a property of the inputs, asserted below, not a measurement of the device.
ORACLE_CASES = [((2000, 5, 64, 6, 5, 3), 3.1786e-03), ((2002, 7, 80, 5, 3, 3), 2.0142e-03), ((2000, 4, 72, 6, 2, 2), 2.0447e-02),
                ((2001, 5, 64, 6, 5, 3), 3.9244e-03)]
MIN_MARGIN = 1e-3


@pytest.mark.parametrize('case,margin', ORACLE_CASES)
def test_several_utterances_per_step_match_the_cpu_oracle(case, margin):
    from oracle import refimpl as R
    seed, k, T, L, W, nbest = case
    bspec = gu.load_beam()[0]
    model, args, vocab, cfg = _f0_model(bspec)
    oracle = R.build_model(cfg)
    gu.perturb_output_layer(oracle.decoder.output_linear.weight, bspec)
    x, lens, y = R.synth_batch(seed, k, T, L, cfg['vocab_size'], True)
    got_margin = bu.oracle_beam_margin(oracle, x, lens, vocab.SOS_ID, W, cfg['tgt_max_len'], vocab.EOS_ID)
    print('seed %d W %d: margin %.4e (recorded %.4e)' % (seed, W, got_margin, margin))
    assert margin >= MIN_MARGIN and got_margin >= MIN_MARGIN and abs(got_margin - margin) <= 0.05 * margin
    U = model.engine.beam_chunk(W)
    assert U > 1 and k >= 2                                                  # several utterances per decoder step
    nw = gu.label_words(vocab.id2label, [vocab.PAD_TOKEN, vocab.SOS_TOKEN, vocab.EOS_TOKEN])
    ref = R.beam_search(oracle, x, lens, vocab.SOS_ID, W, nbest, cfg['tgt_max_len'], nw)
    ref_ids = [[seq for seq, _ in utt] for utt in ref]
    eng, theta = model.engine, model.flat_parameters
    mem, T4 = _memory(model, x, lens, y)
    search = lambda: eng.beam_decode_batch(theta, mem.data_ptr(), k, T4, vocab.SOS_ID, W, nbest, cfg['tgt_max_len'], model._num_words,
                                           vocab.EOS_ID, 1.0)
    dev = search()
    assert [[seq for seq, _ in utt] for utt in dev] == ref_ids
    for utt, rutt in zip(dev, ref):
        for (_, sc), (_, rsc) in zip(utt, rutt):
            assert abs(sc - rsc) <= 1e-4 * max(1.0, abs(rsc))
    # the host-ranked search gives the same answer, and so do the recorded and the replayed command lists of the device-ranked one
    host = [eng.beam_decode(theta, mem.data_ptr() + 4 * b * T4 * eng.hp.d, T4, vocab.SOS_ID, W, nbest, cfg['tgt_max_len'], model._num_words,
                            vocab.EOS_ID, 1.0) for b in range(k)]
    assert [[seq for seq, _ in utt] for utt in host] == ref_ids
    assert search() == dev and search() == dev


@pytest.mark.parametrize('mode', tu.MODES)
def test_evaluate_test_set_on_the_device_reproduces_the_reference(mode, tmp_path):
    import mtl_amd
    t0 = tu.load_t0()
    spec, m = t0['spec'], t0[mode]
    vocab = tu.t0_vocab()
    model = tu.t0_model(mtl_amd, vocab, tgt_max_len=spec['tgt_max_len']).cuda()
    lm = None
    if mode == 'beam_lm':
        path, _ = lu.r0_checkpoint(lu.load_r0(), str(tmp_path / 'lm.pt'))
        lm = mtl_amd.LM(path, argparse.Namespace(cuda=True))
    seen, out = [], io.StringIO()
    with contextlib.redirect_stdout(out):
        res = mtl_amd.evaluate_test_set(model, vocab, tu.t0_loader(t0), tu.eval_args(spec, mode), lm=lm, start_token=vocab.SOS_ID,
                                        on_batch=seen.append)
    lines = [re.sub(r' TOTAL_TIME:[0-9.]+', '', ln) for ln in out.getvalue().splitlines() if ln.startswith('TEST CER:')]
    print('\n'.join(lines))
    assert [[t[k] for k in tu.TOTALS] for t in seen] == m['totals'].tolist()
    assert lines == m['lines']
    assert [res[k] for k in tu.TOTALS] == m['totals'][-1].tolist()
