"""CPU: the host side of LM evaluation -- Dictionary / Corpus against tests/golden/E0.npz (recorded from the reference's
lm/util/data.py by tools/make_golden_lm_eval.py), the checkpoint save_lm_checkpoint writes, the annealing decision of the training
loop and the argument checks of the two evaluation kernels (no device needed)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def e0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'E0.npz'))
    return {k: z[k] for k in z.files}


def _text(a):
    return bytes(a).decode('utf-8')


def _lines(a):
    return _text(a).split('\n')


@pytest.fixture()
def corpus_files(e0, tmp_path):
    paths = {}
    for name in ('train', 'valid', 'test', 'train2'):
        paths[name] = str(tmp_path / (name + '.txt'))
        with open(paths[name], 'w', encoding='utf-8') as f:
            f.write(_text(e0['c/text_' + name]))
    return paths


# ------------------------------------------------------------------------------------------------------------------ Corpus
def test_corpus_matches_the_reference_record(e0, corpus_files):
    import mtl_amd
    assert int(e0['c/real']) == 1                                       # recorded from the real lm/util/data.py Corpus
    assert sum(len(_text(e0['c/text_' + n]).splitlines()) for n in ('train', 'valid', 'test', 'train2')) == 12
    c = mtl_amd.lm.Corpus(corpus_files['train'], corpus_files['valid'], corpus_files['test'])
    assert [c.dictionary.idx2word[i] for i in range(len(c.dictionary))] == _lines(e0['c/words1'])
    for part in ('train', 'valid', 'test'):
        ids, lang = getattr(c, part), getattr(c, part + '_lang')
        assert ids.dtype == torch.int64 and lang.dtype == torch.int64
        assert ids.tolist() == e0['c/' + part].tolist(), part
        assert lang.tolist() == e0['c/%s_lang' % part].tolist(), part
    # chaining: a dictionary passed in is extended, the ids of its words stay
    c2 = mtl_amd.lm.Corpus(corpus_files['train2'], dictionary=c.dictionary)
    assert c2.dictionary is c.dictionary and not hasattr(c2, 'valid') and not hasattr(c2, 'test')
    assert c2.train.tolist() == e0['c/train2'].tolist() and c2.train_lang.tolist() == e0['c/train2_lang'].tolist()
    words2 = _lines(e0['c/words2'])
    assert [c.dictionary.idx2word[i] for i in range(len(c.dictionary))] == words2
    assert words2[:len(_lines(e0['c/words1']))] == _lines(e0['c/words1']) and len(words2) > len(_lines(e0['c/words1']))


def test_corpus_rules(corpus_files):
    import mtl_amd
    c = mtl_amd.lm.Corpus(corpus_files['train'], corpus_files['valid'], corpus_files['test'])
    d = c.dictionary
    assert d.word2idx['<oov>'] == 0 and d.idx2word[0] == '<oov>' and len(d) == len(d.word2idx) == len(d.idx2word)
    eos = d.word2idx['<eos>']
    with open(corpus_files['train'], encoding='utf-8') as f:
        lines = f.read().splitlines()
    assert int((c.train == eos).sum()) == len(lines) and int(c.train[-1]) == eos            # <eos> per line
    assert 'the' in d.word2idx and 'The' not in d.word2idx and 'meeting' in d.word2idx      # lower-cased
    # only the training file adds words; the others map what they do not know to <oov>
    assert 'newword' not in d.word2idx and 'teacher' not in d.word2idx and '取消' not in d.word2idx
    valid_words = [w for line in open(corpus_files['valid'], encoding='utf-8') for w in line.strip().lower().split() + ['<eos>']]
    assert len(valid_words) == c.valid.numel()
    for w, i in zip(valid_words, c.valid.tolist()):
        assert i == d.word2idx.get(w, 0), w
    assert int((c.valid == 0).sum()) == 3 and int((c.train == 0).sum()) == 0
    assert c.valid[valid_words.index('the')] == d.word2idx['the']                           # 'THE' of the valid file
    # langs: 1 for a word that contains a Chinese character -- also for an unknown one
    assert c.valid_lang[valid_words.index('取消')] == 1 and c.valid_lang[valid_words.index('newword')] == 0
    assert c.train_lang[c.train == eos].sum() == 0
    # add_word returns the id and is idempotent
    n = len(d)
    assert d.add_word('the') == d.word2idx['the'] and len(d) == n and d.add_word('zzz') == n and len(d) == n + 1


def test_batchify_free_function_and_method_agree():
    import mtl_amd
    data = torch.arange(23)
    b = mtl_amd.lm.batchify(data, 4)
    assert tuple(b.shape) == (5, 4) and b[:, 0].tolist() == [0, 1, 2, 3, 4] and b[:, 3].tolist() == [15, 16, 17, 18, 19]
    ds = mtl_amd.lm.LMDataset([data], argparse.Namespace(bptt=3, batch_size=4, cuda=False))
    assert torch.equal(ds.task_list[0], b)


# -------------------------------------------------------------------------------------------------------------- checkpoint
def _vocabulary(n):
    return ['<oov>', '<eos>'] + [chr(0x4e00 + i) if i % 2 == 0 else 'w%03d' % i for i in range(2, n)]


def _dictionary(n):
    import mtl_amd
    d = mtl_amd.lm.Dictionary()
    for w in _vocabulary(n):
        d.add_word(w)
    return d


KEYS = {'model_state_dict', 'word2idx', 'idx2word', 'ntoken', 'ninp', 'nhid', 'nlayers', 'dropout', 'tie_weights', 'rnn_type'}


def test_checkpoint_keys_and_tied_state(tmp_path):
    import mtl_amd
    d = _dictionary(40)
    for rnn_type, tied in (('LSTM', False), ('LSTM', True), ('GRU', True)):
        torch.manual_seed(1)
        model = mtl_amd.lm.RNNModel(rnn_type, 40, 16, 16, 2, 0.3, tie_weights=tied)
        path = str(tmp_path / ('%s_%d.pt' % (rnn_type, tied)))
        mtl_amd.lm.save_lm_checkpoint(model, d, path)
        ck = torch.load(path, map_location='cpu', weights_only=False)
        assert set(ck.keys()) == KEYS
        assert (ck['ntoken'], ck['ninp'], ck['nhid'], ck['nlayers'], ck['dropout']) == (40, 16, 16, 2, 0.3)
        assert ck['tie_weights'] is tied and ck['rnn_type'] == rnn_type                    # the real flag, not a constant
        assert ck['word2idx'] == d.word2idx and ck['idx2word'] == d.idx2word
        st = ck['model_state_dict']
        assert list(st.keys()) == list(model.state_dict().keys())
        assert 'encoder.weight' in st and 'decoder.weight' in st                            # both keys, tied or not
        for k, v in model.state_dict().items():
            assert torch.equal(st[k], v) and st[k].is_contiguous() and st[k].untyped_storage().nbytes() == v.numel() * 4, k
        if tied:
            assert torch.equal(st['encoder.weight'], st['decoder.weight'])


def test_lm_loads_a_saved_untied_lstm(tmp_path):
    import mtl_amd
    d = _dictionary(40)
    torch.manual_seed(2)
    model = mtl_amd.lm.RNNModel('LSTM', 40, 16, 24, 2, 0.3)
    path = str(tmp_path / 'lm.pt')
    mtl_amd.lm.save_lm_checkpoint(model, d, path)
    lm = mtl_amd.LM(path, argparse.Namespace(cuda=False))
    assert lm.word2idx == d.word2idx and not lm.model.training
    assert (lm.model.ntoken, lm.model.ninp, lm.model.nhid, lm.model.nlayers) == (40, 16, 24, 2)
    want = model.state_dict()
    got = lm.model.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert torch.equal(got[k], want[k]), k
    ids, oov = lm.seq_to_tensor('w003 %s nope' % chr(0x4e00 + 4))
    assert ids.tolist() == [3, 4, 0, 1] and oov == 1


def test_checkpoint_of_the_golden_record(e0, tmp_path):
    """E0 (b): the reference's utils/lm.py LM loaded a file written by save_lm_checkpoint for this very model"""
    import mtl_amd
    spec = json.loads(_text(e0['spec']))
    H = spec['ckpt']['nhid']
    torch.manual_seed(spec['seed'])
    model = mtl_amd.lm.RNNModel('LSTM', spec['ntoken'], H, H, spec['nlayers'], spec['dropout'], True)
    path = str(tmp_path / 'lm.pt')
    mtl_amd.lm.save_lm_checkpoint(model, _dictionary(spec['ntoken']), path)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ck.keys()) == _lines(e0['b/keys'])
    st = ck['model_state_dict']
    assert list(st.keys()) == _lines(e0['b/state_names'])
    assert [','.join(str(v) for v in t.shape) for t in st.values()] == _lines(e0['b/state_shapes'])
    assert [str(t.dtype) for t in st.values()] == _lines(e0['b/state_dtypes'])
    assert e0['b/scores'].shape == (3,) and np.isfinite(e0['b/scores']).all() and e0['b/oov'].tolist() == [0, 1, 0]


# --------------------------------------------------------------------------------------------------------------- annealing
def test_anneal_step_decisions():
    import mtl_amd
    step = mtl_amd.lm.anneal_step
    assert step(None, 0, 20.0, 5.0) == (5.0, 0, 20.0, True, False)               # first value: saved
    assert step(0, 3, 20.0, 5.0) == (5.0, 0, 20.0, True, False)                  # `not best`: the reference starts from 0
    assert step(5.0, 2, 20.0, 4.5) == (4.5, 0, 20.0, True, False)                # improvement resets the counter
    assert step(5.0, 0, 20.0, 5.0) == (5.0, 1, 5.0, False, False)                # equal is no improvement: lr / 4
    assert step(5.0, 1, 5.0, 6.0, patience=5) == (5.0, 2, 1.25, False, False)
    assert step(5.0, 4, 20.0, 6.0) == (5.0, 5, 5.0, False, True)                 # default patience 5
    best, counter, lr, stops = None, 0, 16.0, []
    for val in (3.0, 3.5, 2.9, 3.0, 3.1, 3.2):
        best, counter, lr, save, stop = step(best, counter, lr, val, patience=3)
        stops.append((save, stop))
    assert stops == [(True, False), (False, False), (True, False), (False, False), (False, False), (False, True)]
    assert (best, counter, lr) == (2.9, 3, 16.0 / 4 ** 4)


def test_train_keeps_its_signature_defaults():
    import inspect
    import mtl_amd
    sig = inspect.signature(mtl_amd.lm.LMMetaTrainer.train)
    want = dict(log_interval=200, valid_interval=None, val_data=None, test_data=None, save_path=None, dictionary=None, eval_bptt=None,
                patience=5)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == want
    sig = inspect.signature(mtl_amd.lm.LMEngine.evaluate)
    assert list(sig.parameters)[1:] == ['theta', 'source', 'bptt', 'lang', 'eos_id', 'chunk_windows', 'rows']


def test_no_cpu_fallback():
    import mtl_amd
    model = mtl_amd.lm.RNNModel('LSTM', 20, 8, 8, 1, 0.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mtl_amd.lm.evaluate(model, torch.zeros(6, 2, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mtl_amd.lm.evaluate_test(model, torch.zeros(6, 2, dtype=torch.int64), _dictionary(20), 3)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_kernel_argument_validation_without_gpu():
    import mtl_amd
    L = mtl_amd._lib.lib()
    a, EINVAL = 4096, -22                                                # any non-null address: rejected calls launch nothing
    text = open(os.path.join(ROOT, 'include', 'mtl_hip.h')).read()
    assert '#define MTL_NLL_MAX_KEYS 4096' in text and mtl_amd.lm.MAX_KEYS == 4096
    assert L.mtl_nll_key_sum_workspace(70001, 4096) >= 69 * 4096 * 12 and L.mtl_nll_key_sum_workspace(1, 1) >= 12
    assert L.mtl_nll_key_sum_workspace(10, 4097) == EINVAL and L.mtl_nll_key_sum_workspace(0, 4) == EINVAL
    assert L.mtl_nll_key_sum_workspace(10, 0) == EINVAL
    ws = 1 << 20

    def key_sum(**kw):
        p = dict(row=a, key=a, seg=1, R=100, nkey=4, sum=a, count=a, ws=a, ws_bytes=ws)
        p.update(kw)
        return L.mtl_nll_key_sum(None, p['row'], p['key'], p['seg'], p['R'], p['nkey'], p['sum'], p['count'], p['ws'], p['ws_bytes'])
    assert key_sum(nkey=4097, ws_bytes=1 << 30) == EINVAL
    assert key_sum(nkey=0) == EINVAL
    assert key_sum(R=0) == EINVAL and key_sum(R=-5) == EINVAL
    for name in ('row', 'sum', 'count', 'ws'):
        assert key_sum(**{name: None}) == EINVAL, name
    assert key_sum(key=None, seg=0) == EINVAL and key_sum(key=None, seg=-1) == EINVAL
    assert key_sum(ws_bytes=47) == EINVAL                                # at least one block x 4 keys x 12 bytes
    assert key_sum(ws=a + 4) == EINVAL                                   # fp64 partials: 8-byte aligned

    def keys(**kw):
        p = dict(ids=a, target=a, lang=a, eos=1, R=10, V=150, key=a)
        p.update(kw)
        return L.mtl_lm_switch_keys(None, p['ids'], p['target'], p['lang'], p['eos'], p['R'], p['V'], p['key'])
    for name in ('ids', 'target', 'lang', 'key'):
        assert keys(**{name: None}) == EINVAL, name
    assert keys(R=0) == EINVAL and keys(V=0) == EINVAL
    for name in ('mtl_lm_switch_keys', 'mtl_nll_key_sum'):
        assert L.mtl_cmdlist_opcode(name.encode()) >= 0, name            # recordable
    assert L.mtl_cmdlist_opcode(b'mtl_nll_key_sum_workspace') == -1
