"""Generate tests/golden/E0.npz: LM evaluation, checkpoint and corpus records of the REAL reference.

Runs only where the reference checkout exists (it imports the reference's own modules and copies nothing).  Records
  (a) the evaluate loop of lm/main_meta_transfer.py:214-267 / lm/test.py:189-241 (those files are scripts and cannot be imported, so the
      loop is restated here) around the real `lm/model/rnn_model.py:RNNModel` on the CPU, cast to fp64 after its fp32 initialisation:
      per window `len(data) * CrossEntropyLoss()` and the total `/ len(data_source)`, for every stream of SPEC['streams'] and the models
      LSTM untied, LSTM tied and GRU at both hidden sizes.  Every model is the seeded initialisation plus the seeded perturbation of
      `perturb` (the plain initialisation predicts a nearly uniform distribution: every window would score log V);
  (b) the real `utils/lm.py:LM` loading a checkpoint that mtl_amd.lm.save_lm_checkpoint wrote (a tied LSTM: that class always builds
      an LSTM, and the reference's converter always writes tie_weights=True): names, shapes and dtypes of the file's tensors and
      LM.evaluate of three strings;
  (c) the real `lm/util/data.py:Corpus` (third-party imports that are absent stubbed here) on the 12-line fixture text below: ids,
      langs and the word list, for a train / valid / test triple and for a second corpus chained through the first one's dictionary.

    python tools/make_golden_lm_eval.py
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import bootstrap_reference  # noqa: E402

SPEC = dict(seed=4321, ntoken=150, nlayers=2, dropout=0.2, corpus_seed=5, noise_seed=17, noise=dict(enc=0.5, dec=1.0, bias=1.5),
            streams=[[70, 3, 5], [41, 1, 5], [330, 10, 7]], hidden=[32, 128],
            models=dict(lstm=['LSTM', False], lstm_tied=['LSTM', True], gru=['GRU', False]),
            ckpt=dict(nhid=32, strings=['w003 丂 w005 丄', '丄 w007 unknownword', 'w149 w003']))

TRAIN = """你 好 hello world
我 要 去  school today
The Meeting 是 明天
ok 那 我们 go 吧
"""
VALID = """你 好 teacher
newword 我 要 go
明天 THE meeting 取消
"""
TEST = """hello 你 们 好
school 是 什么
   我们 去   吧 ok
"""
TRAIN2 = """second corpus 你 好
brand new 词 hello
"""


def vocabulary(n):
    """id 0 <oov>, 1 <eos>, then even ids a CJK character and odd ids a Latin word"""
    return ['<oov>', '<eos>'] + [chr(0x4e00 + i) if i % 2 == 0 else 'w%03d' % i for i in range(2, n)]


def perturb(model, torch):
    """seeded noise on the embedding, the vocabulary projection (unless tied) and its bias, drawn in this order"""
    g = torch.Generator().manual_seed(SPEC['noise_seed'])
    with torch.no_grad():
        model.encoder.weight += SPEC['noise']['enc'] * torch.randn(model.encoder.weight.shape, generator=g)
        if model.decoder.weight is not model.encoder.weight:
            model.decoder.weight += SPEC['noise']['dec'] * torch.randn(model.decoder.weight.shape, generator=g)
        model.decoder.bias += SPEC['noise']['bias'] * torch.randn(model.decoder.bias.shape, generator=g)


def evaluate(model, source, bptt, torch):
    """the reference's loop -> (window losses len(data) * criterion, total / len(source))"""
    crit = torch.nn.CrossEntropyLoss()
    model.eval()
    hidden = model.init_hidden(source.size(1))
    hidden = tuple(h.double() for h in hidden) if isinstance(hidden, tuple) else hidden.double()
    wins, total = [], 0
    with torch.no_grad():
        for i in range(0, source.size(0) - 1, bptt):
            seq_len = min(bptt, len(source) - 1 - i)
            data, targets = source[i:i + seq_len], source[i + 1:i + 1 + seq_len].reshape(-1)
            output, hidden = model(data, hidden)
            w = len(data) * crit(output.view(-1, output.size(-1)), targets)
            wins.append(float(w))
            total = total + w
    return np.array(wins, dtype=np.float64), float(total) / len(source)


def main():
    torch = bootstrap_reference()
    sys.path.insert(0, '/root/reference/lm')
    for name in ('scipy', 'scipy.spatial', 'scipy.spatial.distance', 'tqdm'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__dict__.update(spatial=None, cosine=None, tqdm=lambda x, **k: x)
    from model.rnn_model import RNNModel
    import utils.lm as ref_lm
    import mtl_amd
    torch.set_num_threads(8)
    enc_str = lambda lst: np.frombuffer('\n'.join(lst).encode('utf-8'), dtype=np.uint8)
    store = {'spec': np.frombuffer(json.dumps(SPEC).encode(), dtype=np.uint8)}

    # (a)
    V = SPEC['ntoken']
    for H in SPEC['hidden']:
        for key, (rnn_type, tied) in SPEC['models'].items():
            torch.manual_seed(SPEC['seed'])
            model = RNNModel(rnn_type, V, H, H, SPEC['nlayers'], SPEC['dropout'], tied)
            perturb(model, torch)
            h = hashlib.sha256()
            for _, p in model.named_parameters():
                h.update(p.detach().numpy().tobytes())
            store['a/%s_h%d/theta_sha256' % (key, H)] = np.frombuffer(h.hexdigest().encode(), dtype=np.uint8)
            model = model.double()
            for N, B, bptt in SPEC['streams']:
                data = mtl_amd.lm.synth_corpus(SPEC['corpus_seed'], V, N)
                source = data.narrow(0, 0, (N // B) * B).view(B, -1).t().contiguous()
                wins, total = evaluate(model, source, bptt, torch)
                store['a/%s_h%d/n%d/window_loss' % (key, H, N)], store['a/%s_h%d/n%d/loss' % (key, H, N)] = wins, np.float64(total)
                print('(a) %-9s H=%3d N=%3d B=%2d bptt=%d: %2d windows, loss %.6f' % (key, H, N, B, bptt, len(wins), total))

    # (b)
    words = vocabulary(V)
    d = mtl_amd.lm.Dictionary()
    for w in words:
        d.add_word(w)
    torch.manual_seed(SPEC['seed'])
    ours = mtl_amd.lm.RNNModel('LSTM', V, SPEC['ckpt']['nhid'], SPEC['ckpt']['nhid'], SPEC['nlayers'], SPEC['dropout'], True)
    perturb(ours, torch)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'lm.pt')
        mtl_amd.lm.save_lm_checkpoint(ours, d, path)
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        lm = ref_lm.LM(path, argparse.Namespace(cuda=False))
    state = ckpt['model_state_dict']
    store['b/keys'] = enc_str(sorted(ckpt.keys()))
    store['b/state_names'] = enc_str(list(state.keys()))
    store['b/state_shapes'] = enc_str([','.join(str(v) for v in t.shape) for t in state.values()])
    store['b/state_dtypes'] = enc_str([str(t.dtype) for t in state.values()])
    scores, oovs = [], []
    with torch.no_grad():
        for s in SPEC['ckpt']['strings']:
            sc, oov = lm.evaluate(s)
            scores.append(float(sc))
            oovs.append(int(oov))
    store['b/scores'], store['b/oov'] = np.array(scores, dtype=np.float32), np.array(oovs, dtype=np.int64)
    print('(b) %d tensors, scores %s, oov %s' % (len(state), scores, oovs))

    # (c)
    try:
        from util.data import Corpus
        store['c/real'] = np.int64(1)
    except Exception as e:                                              # pinned to the restatement only: "parity unpinned"
        print('(c) the reference Corpus does not import (%r): recording the restatement' % (e,))
        Corpus = mtl_amd.lm.Corpus
        store['c/real'] = np.int64(0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for name, text in (('train', TRAIN), ('valid', VALID), ('test', TEST), ('train2', TRAIN2)):
            paths[name] = os.path.join(tmp, name + '.txt')
            with open(paths[name], 'w', encoding='utf-8') as f:
                f.write(text)
        c1 = Corpus(paths['train'], paths['valid'], paths['test'])
        store['c/words1'] = enc_str([c1.dictionary.idx2word[i] for i in range(len(c1.dictionary))])
        c2 = Corpus(paths['train2'], dictionary=c1.dictionary)
    for part in ('train', 'valid', 'test'):
        store['c/' + part], store['c/%s_lang' % part] = getattr(c1, part).numpy(), getattr(c1, part + '_lang').numpy()
    store['c/train2'], store['c/train2_lang'] = c2.train.numpy(), c2.train_lang.numpy()
    store['c/words2'] = enc_str([c2.dictionary.idx2word[i] for i in range(len(c2.dictionary))])
    for name, text in (('train', TRAIN), ('valid', VALID), ('test', TEST), ('train2', TRAIN2)):
        store['c/text_' + name] = np.frombuffer(text.encode('utf-8'), dtype=np.uint8)
    print('(c) real=%d: %d + %d words, %d / %d / %d / %d tokens' % (int(store['c/real']), len(c1.dictionary) - 0, len(c2.dictionary),
                                                                   len(c1.train), len(c1.valid), len(c1.test), len(c2.train)))

    out = os.path.join(ROOT, 'tests', 'golden', 'E0.npz')
    np.savez_compressed(out, **store)
    print('E0 written: %d bytes' % os.path.getsize(out))


if __name__ == '__main__':
    main()
