"""CPU: the host side of beam search with LM rescoring, pinned to tests/golden/R0.npz (recorded from the reference's
modules/decoder.py:248-264 and utils/lm.py): word segmentation, the strings handed to LM.evaluate, word and OOV counts, checkpoint
loading, and the argument checks of the fused LM NLL kernel (no device needed)."""
import argparse
import random

import pytest

from tests import lm_rescore_util as lu


@pytest.fixture(scope='module')
def r0():
    return lu.load_r0()


def test_word_segments_per_language():
    import mtl_amd
    seg = mtl_amd.get_word_segments_per_language
    assert mtl_amd.is_chinese_char('中') and not mtl_amd.is_chinese_char('a') and not mtl_amd.is_chinese_char(' ')
    assert mtl_amd.is_contain_chinese_word('ab中') and not mtl_amd.is_contain_chinese_word('abc')
    assert seg('') == ['']
    assert seg('hello world') == ['hello world']
    assert seg('我 们 go home 好') == ['我 们', 'go home', '好']
    assert seg('a  b') == ['a  b']                          # '' words from a double space stay in their run
    assert seg('中  文') == ['中', '', '文']                   # ... and an empty word counts as English
    assert seg(' x') == ['x'] and seg('中 ') == ['中', '']           # (a leading '' word is absorbed)


def _ref_segments(seq):
    """utils/data.py:84-127 restated literally (loop with the reference's five branches)"""
    import unicodedata
    zh = lambda w: any(unicodedata.category(c) == 'Lo' for c in w)
    cur, temp, out = -1, '', []
    for word in seq.split(' '):
        if zh(word):
            if cur == -1:
                cur, temp = 1, word
            elif cur == 0:
                cur = 1
                out.append(temp)
                temp = word
            else:
                temp = temp + (' ' if temp != '' else '') + word
        else:
            if cur == -1:
                cur, temp = 0, word
            elif cur == 1:
                cur = 0
                out.append(temp)
                temp = word
            else:
                temp = temp + (' ' if temp != '' else '') + word
    out.append(temp)
    return out


def test_word_segments_random_strings():
    import mtl_amd
    rnd = random.Random(5)
    for _ in range(5000):
        s = ''.join(rnd.choice(['a', 'bc', ' ', '  ', '中', '文', 'é']) for _ in range(rnd.randint(0, 10)))
        assert mtl_amd.get_word_segments_per_language(s) == _ref_segments(s), repr(s)


def test_strings_handed_to_the_lm_match_the_reference(r0):
    """every ended hypothesis of R0 -> lm_string: exactly the strings the reference's LM.evaluate received (the spy's record)"""
    import mtl_amd
    vocab = lu.r0_vocab(r0)
    assert len(r0['ended_ids']) == sum(r0['ended_count'])
    mine = [mtl_amd.lm_string(y, vocab) for y in r0['ended_ids']]
    assert sorted(s for s in mine if s) == sorted(r0['lm_seen'])
    # mixed scripts occur: English words and single Chinese characters
    words = [w for s in r0['lm_seen'] for w in s.split()]
    assert any(mtl_amd.is_contain_chinese_word(w) for w in words) and any(w.isascii() and len(w) > 1 for w in words)


def test_word_and_oov_counts_of_hand_made_hypotheses(r0, tmp_path):
    import mtl_amd
    vocab = lu.r0_vocab(r0)
    path, _ = lu.r0_checkpoint(r0, str(tmp_path / 'lm.pt'))
    lm = mtl_amd.LM(path, argparse.Namespace(cuda=False))
    for yseq, nw, oov, sc in zip(r0['hand_ids'], r0['hand_num_words'], r0['hand_oov'], r0['hand_score']):
        s = mtl_amd.lm_string(yseq, vocab)
        if s == '':
            assert (nw, oov, sc) == (0, 0, -999)
            assert mtl_amd.calculate_lm_score(yseq, lm, vocab) == (-999, 0, 0)        # no LM call: no device needed
            continue
        assert len(s.split()) + 1 == nw                    # the LM's word count + 1, not the label string's
        assert lm.seq_to_tensor(s)[1] == oov
    kinds = [mtl_amd.lm_string(y, vocab) for y in r0['hand_ids']]
    assert '' in kinds and any(o == len(s.split()) > 0 for s, o in zip(kinds, r0['hand_oov']))      # empty and all-OOV cases


def test_lm_checkpoint_loading(r0, tmp_path):
    import torch
    import mtl_amd
    path, sha = lu.r0_checkpoint(r0, str(tmp_path / 'lm.pt'))
    assert sha == r0['lm_sha256']                        # lm.RNNModel draws the reference's initialisation bit for bit
    lm = mtl_amd.LM(path, argparse.Namespace(cuda=False))
    assert lm.word2idx['<oov>'] == 0 and lm.idx2word == r0['words']
    assert lm.model.nhid == r0['spec']['lm_nhid'] and lm.model.nlayers == r0['spec']['lm_nlayers'] and not lm.model.training
    sd = torch.load(path, weights_only=False)['model_state_dict']
    for k, v in lm.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    ids, oov = lm.seq_to_tensor('r 丒 zz')
    assert ids.tolist()[-1] == lm.word2idx['<eos>'] and oov == sum(w not in lm.word2idx for w in ['r', '丒', 'zz'])
    with pytest.raises(RuntimeError, match='MI355X'):
        lm.model._need_engine()                          # no CPU fallback
    tied, _ = lu.r0_checkpoint(r0, str(tmp_path / 'tied.pt'), tie_weights=True)
    with pytest.raises(NotImplementedError, match='tie_weights'):
        mtl_amd.LM(tied, argparse.Namespace(cuda=False))
    gru, _ = lu.r0_checkpoint(r0, str(tmp_path / 'gru.pt'), rnn_type='GRU')
    with pytest.raises(NotImplementedError, match='LSTM'):
        mtl_amd.LM(gru, argparse.Namespace(cuda=False))


def test_lm_nll_argument_validation():
    import __graft_entry__ as ge
    L = ge.build()._lib.lib()
    ws = L.mtl_lm_nll_workspace(256, 30011)
    assert ws > 0 and ws % 12 == 0 and L.mtl_lm_nll_workspace(0, 10) == 0 and L.mtl_lm_nll_workspace(10, 0) == 0
    assert L.mtl_lm_nll_workspace(1, 150) >= 12
    p = 4096                                              # (never dereferenced: every call below is rejected before a launch)
    ok = dict(x=p, ldx=200, W=p, bias=p, tgt=p, R=256, H=200, V=30011, B=32, row=p, seq=p, ws=p, wsb=ws)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mtl_lm_nll_fwd(None, a['x'], a['ldx'], a['W'], a['bias'], a['tgt'], a['R'], a['H'], a['V'], a['B'], a['row'], a['seq'],
                                a['ws'], a['wsb'])
    for bad in (dict(x=None), dict(W=None), dict(tgt=None), dict(row=None), dict(ws=None), dict(R=0), dict(H=0), dict(V=0), dict(B=0),
                dict(B=30), dict(ldx=199), dict(wsb=ws - 1), dict(ws=p + 2)):
        assert call(**bad) == -22, bad


def test_rescoring_requires_an_lm():
    import mtl_amd
    m = mtl_amd.Transformer.__new__(mtl_amd.Transformer)
    with pytest.raises(ValueError, match='lm='):
        mtl_amd.Transformer.evaluate(m, None, None, None, argparse.Namespace(), beam_search=True, lm_rescoring=True, lm=None)
