"""CPU: the drop-ins of the reference's test.py (calculate_wer, calculate_cer_en_zh, compute_num_params, evaluate_test_set) against
the reference's recorded evaluation (tests/golden/T0.npz, tools/make_golden_test_eval.py), and the argument checks of the beam
search entry points (no device needed)."""
import inspect
import io
import contextlib
import random
import re

import numpy as np
import pytest
import torch

from tests import eval_util as tu


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope='module')
def t0():
    return tu.load_t0()


def _dp(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[-1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def _wer_dp(s1, s2):
    return _dp(s1.split(), s2.split())


def _is_zh(word):
    return any('一' <= c <= '鿿' for c in word)


def _en_zh_dp(s1, s2):
    """plain restatement: words (split on single spaces) grouped into runs of one language, runs space-joined, the runs of a language
    concatenated without a separator"""
    def seqs(s):
        runs, lang = [], None
        for w in s.split(' '):
            z = _is_zh(w)
            if lang is None or z != lang:
                runs.append([z, w])
            else:
                runs[-1][1] = runs[-1][1] + (' ' if runs[-1][1] != '' else '') + w
            lang = z
        return ''.join(r[1] for r in runs if not r[0]), ''.join(r[1] for r in runs if r[0])
    (en1, zh1), (en2, zh2) = seqs(s1), seqs(s2)
    return _dp(en1, en2), _dp(zh1, zh2), len(en2), len(zh2)


def test_wer_and_per_language_cer_reproduce_the_reference(built, t0):
    for mode in tu.MODES:
        m = t0[mode]
        for hyp, gold, row in zip(m['hyp'], m['gold'], m['per_utt']):
            wer, cer, en_cer, zh_cer, en_char, zh_char, hyp_char, words, chars = (int(v) for v in row)
            assert built.calculate_wer(hyp, gold) == wer
            assert built.calculate_cer(hyp.strip(), gold.strip()) == cer
            assert built.calculate_cer_en_zh(hyp, gold) == (en_cer, zh_cer, en_char, zh_char)
            assert (len(hyp), len(gold.split(' ')), len(gold)) == (hyp_char, words, chars)


def test_wer_and_per_language_cer_against_plain_dp(built):
    rnd = random.Random(0)
    alphabet = 'abcde' + '一丁七三' + '   '
    for _ in range(200):
        a = ''.join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 24)))
        b = ''.join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 24)))
        assert built.calculate_wer(a, b) == _wer_dp(a, b), (a, b)
        assert built.calculate_cer_en_zh(a, b) == _en_zh_dp(a, b), (a, b)
    assert built.calculate_wer('', '') == 0 and built.calculate_wer('a b', '') == 2


def test_compute_num_params(built):
    lin = torch.nn.Linear(3, 5)
    lin.bias.requires_grad_(False)
    assert built.compute_num_params(lin) == (15, 5)


@pytest.mark.parametrize('mode', tu.MODES)
def test_evaluate_test_set_reproduces_the_reference_totals_and_line(built, t0, mode):
    """a stub model hands out T0's recorded strings: the accumulation, the hypothesis indexing and the printed line are the reference's"""
    m, spec = t0[mode], t0['spec']
    vocab = tu.t0_vocab()
    calls = []

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.i = 0

        def evaluate(self, src, src_lengths, trg, args, **kw):
            calls.append(kw)
            n = src.shape[0]
            out = (None, m['hyp'][self.i:self.i + n], m['gold'][self.i:self.i + n])
            self.i += n
            return out
    loader = [(torch.zeros(b['k'], 1, 161, b['T']), torch.zeros(b['k'], b['L'], dtype=torch.int64), None, torch.zeros(b['k']), None)
              for b in spec['batches']]
    args = tu.eval_args(spec, mode)
    seen = []
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = built.evaluate_test_set(Stub(), vocab, loader, args, lm=None, start_token=vocab.SOS_ID, on_batch=seen.append)
    lines = [re.sub(r' TOTAL_TIME:[0-9.]+', '', ln) for ln in out.getvalue().splitlines() if ln.startswith('TEST CER:')]
    assert lines == m['lines']
    assert [[t[k] for k in tu.TOTALS] for t in seen] == m['totals'].tolist()
    assert [res[k] for k in tu.TOTALS] == m['totals'][-1].tolist()
    assert re.sub(r' TOTAL_TIME:[0-9.]+', '', res['line']) == m['lines'][-1]
    assert res['cer'] == res['total_cer'] * 100 / res['total_char'] and res['wer'] == res['total_wer'] * 100 / res['total_word']
    assert 'TOTAL_TIME:' in res['line'] and res['total_time'] >= 0
    # the reference's keyword set, plus the new one
    assert set(calls[0]) == {'lm_rescoring', 'lm', 'lm_weight', 'beam_search', 'beam_width', 'beam_nbest', 'c_weight', 'start_token', 'verbose',
                             'device_ranking'}
    assert calls[0]['device_ranking'] is True and calls[0]['start_token'] == vocab.SOS_ID


def test_beam_entry_points_reject_bad_arguments_without_a_device(built):
    L = built._lib.lib()
    ok = dict(logits=64, lse=64, state=64, tok=64, parent=64, i=0, T4=16, U=3, W=5, V=100, S=16, eos=2)      # (never launched: see below)

    def rank(**kw):
        a = dict(ok, **kw)
        return L.mtl_beam_rank(None, a['logits'], a['lse'], a['state'], a['tok'], a['parent'], a['i'], a['T4'], a['U'], a['W'], a['V'], a['S'],
                               a['eos'])
    assert rank(state=None) == -22 and rank(logits=None) == -22 and rank(lse=None) == -22 and rank(tok=None) == -22 and rank(parent=None) == -22
    assert rank(i=-1) == -22 and rank(i=16) == -22
    assert rank(W=0) == -22 and rank(W=9) == -22                              # MTL_BEAM_MAX_W = 8
    assert rank(V=4) == -22 and rank(V=(1 << 20) + 1) == -22                  # V >= W, MTL_BEAM_MAX_V
    assert rank(S=4097) == -22 and rank(U=0) == -22 and rank(U=65) == -22 and rank(eos=100) == -22 and rank(T4=0) == -22
    assert L.mtl_beam_state_words(3, 5, 16) == 4 * 3 + 3 * 5 + 7 * 3 * 16 * 5
    assert L.mtl_beam_state_words(3, 9, 16) == -22 and L.mtl_beam_state_words(3, 5, 4097) == -22

    def gather(caches=64, ncache=2, parent=64, tmp=64, tmp_floats=2 * 15 * 4 * 128, rows=15, t=4, width=128, stride=16 * 128):
        return L.mtl_beam_gather(None, caches, ncache, parent, tmp, tmp_floats, rows, t, width, stride)
    assert gather(caches=None) == -22 and gather(parent=None) == -22 and gather(tmp=None) == -22
    assert gather(t=0) == -22 and gather(rows=0) == -22 and gather(ncache=0) == -22 and gather(ncache=65) == -22
    assert gather(width=126) == -22 and gather(stride=3 * 128) == -22 and gather(tmp_floats=100) == -22 and gather(tmp=68) == -22
    # both are recordable
    assert L.mtl_cmdlist_opcode(b'mtl_beam_rank') >= 0 and L.mtl_cmdlist_opcode(b'mtl_beam_gather') >= 0
    assert L.mtl_cmdlist_opcode(b'mtl_beam_state_words') == -1


def test_evaluate_accepts_device_ranking_and_keeps_its_argument_checks(built):
    sig = inspect.signature(built.Transformer.evaluate)
    assert sig.parameters['device_ranking'].default is False
    assert list(sig.parameters)[-1] == 'device_ranking'                     # appended: positional callers are untouched
    sig = inspect.signature(built.evaluate_test_set)
    assert list(sig.parameters)[:6] == ['model', 'vocab', 'test_loader', 'args', 'lm', 'start_token'] and sig.parameters['device_ranking'].default is True
    import argparse
    vocab = tu.t0_vocab()
    model = tu.t0_model(built, vocab, perturb=False)
    x, y = torch.zeros(1, 1, 161, 32), torch.ones(1, 3, dtype=torch.int64) * 5
    args = argparse.Namespace(beam_width=3, beam_nbest=1, tgt_max_len=50)
    for dr in (False, True):
        with pytest.raises(ValueError, match='lm_rescoring=True needs lm='):
            model.evaluate(x, [32], y, args, beam_search=True, lm_rescoring=True, device_ranking=dr)
        with pytest.raises(RuntimeError, match='no CPU'):
            model.evaluate(x, [32], y, args, beam_search=True, device_ranking=dr)


def test_beam_unpack_rebuilds_sequences_from_back_pointers(built):
    from mtl_amd.engine import beam_unpack
    from tests import beam_util as bu
    U, W, S, eos, V = 2, 3, 4, 2, 11
    rng = np.random.RandomState(3)
    st = bu.new_state(U, W, S, [1, 1], [[0.0], [0.0]])
    tok = np.full(U * W, eos, dtype=np.int64)
    par = np.zeros(U * W, dtype=np.int32)
    # replay the search on the host as PassEngine.beam_decode keeps it (lists of yseq per live row) next to the state
    live = [[[1]] for _ in range(U)]
    ended = [[] for _ in range(U)]
    for i in range(S):
        logits = rng.randn(U * W, V).astype(np.float32)
        logits[:, eos] += 1.0
        lse = np.log(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
        before = st.copy()
        bu.rank_position(st, logits, lse, tok, par, i, S, U, W, V, S, eos)
        o_score, o_bp, o_tk, o_en, _ = bu.state_offsets(U, W, S)
        for u in range(U):
            if before[4 * u + 1]:
                continue
            for e in range(int(before[4 * u + 2]), int(st[4 * u + 2])):
                pos, _sc, row, t, forced = st[o_en + 5 * (u * S * W + e):o_en + 5 * (u * S * W + e) + 5]
                ended[u].append(live[u][row] + [int(t)] + ([eos] if forced else []))
            n = int(st[4 * u])
            live[u] = [live[u][int(st[o_bp + (u * S + i) * W + r])] + [int(st[o_tk + (u * S + i) * W + r])] for r in range(n)]
    got = beam_unpack(st, U, W, S, 1, eos)
    assert [[h['yseq'] for h in utt] for utt in got] == ended
    assert all(len(utt) >= 1 and utt[-1]['yseq'][-1] == eos for utt in got)
    assert all(h['score'].dtype == np.float32 for utt in got for h in utt)
