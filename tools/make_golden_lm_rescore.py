"""Generate tests/golden/R0.npz: beam search with LM rescoring (modules/decoder.py:248-264, utils/lm.py) of the REAL reference.

Runs only where the reference checkout exists (it imports the reference's own modules through oracle/make_golden.py's bootstrap,
never copies them).  Model: the F0 model with the B0 perturbation of its vocabulary projection, relabelled with a vocabulary that
mixes CJK characters, Latin letters and ' ' (so hypotheses hold English words and Chinese characters); LM: a small seeded 2-layer
LSTM (the reference's RNNModel, rebuilt bit-identically from the recorded seed by lm.RNNModel) whose word list is harvested from a
rescoring-free beam run and thinned, so that in-vocabulary and out-of-vocabulary words both occur.

    python tools/make_golden_lm_rescore.py
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import bootstrap_reference, FIXTURES  # noqa: E402

SPACE_AT = 47                    # the label of an id B0's perturbed model emits often: ' '
SPEC = dict(seed=500, k=6, T=64, L=8, beam_width=3, nbest=3, noise_seed=7, noise=0.5, eos_from=47, eos_gain=1.02,
            lm_seed=2024, lm_ninp=128, lm_nhid=128, lm_nlayers=2, lm_dropout=0.2, lm_ntoken=150, lm_noise_seed=11, lm_noise=1.5,
            lm_weight=0.6, c_weight=1.0)


def labels():
    """60 non-special labels: one ' ', 26 Latin letters and 33 CJK characters, interleaved"""
    out, latin, cjk = [], iter('abcdefghijklmnopqrstuvwxyz'), iter(chr(0x4e00 + i) for i in range(100))
    for i in range(FIXTURES['F0']['cfg']['vocab_size'] - 4):
        out.append(' ' if i == SPACE_AT else (next(latin) if i % 2 and i < 53 else next(cjk)))
    return out


def lm_words(hyps, lm_string):
    """words of a rescoring-free beam run (as calculate_lm_score would hand them over), every other one kept"""
    words = []
    for s in hyps:
        for w in lm_string(s).split():
            if w not in words:
                words.append(w)
    return words[::2]


def main():
    torch = bootstrap_reference()
    from utils.data import Vocab
    from utils.functions import init_transformer_model
    import utils.lm as ref_lm
    import modules.decoder as ref_dec
    from oracle.refimpl import synth_batch
    import mtl_amd

    cfg = FIXTURES['F0']['cfg']
    labs = labels()
    vocab = Vocab()
    for c in labs:
        vocab.add_token(c)
        vocab.add_label(c)
    assert len(vocab.id2label) == cfg['vocab_size'], len(vocab.id2label)
    args = argparse.Namespace(
        feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
        num_enc_layers=cfg['num_enc_layers'], num_dec_layers=cfg['num_dec_layers'], num_heads=cfg['num_heads'],
        dim_model=cfg['dim_model'], dim_key=cfg['dim_key'], dim_value=cfg['dim_value'], dim_inner=cfg['dim_inner'],
        dim_emb=cfg['dim_emb'], src_max_len=cfg['src_max_len'], tgt_max_len=cfg['tgt_max_len'], dropout=0.0,
        emb_trg_sharing=False, label_smoothing=0.0, name='golden_R0', cuda=False, beam_width=SPEC['beam_width'],
        beam_nbest=SPEC['nbest'])
    torch.manual_seed(123456)
    torch.set_num_threads(8)
    model = init_transformer_model(args, vocab, is_factorized=False, r=cfg['r'])
    g = torch.Generator().manual_seed(SPEC['noise_seed'])
    W = model.decoder.output_linear.weight
    W.data += SPEC['noise'] * torch.randn(W.shape, generator=g)
    W.data[2] = SPEC['eos_gain'] * W.data[SPEC['eos_from']]
    model.eval()
    x, lens, y = synth_batch(SPEC['seed'], SPEC['k'], SPEC['T'], SPEC['L'], cfg['vocab_size'], variable=True)
    to_str = lambda yseq: ''.join(vocab.id2label[int(c)] for c in yseq)

    with torch.no_grad():
        f = model.conv(x)
        sz = f.size()
        enc, _ = model.encoder(f.view(sz[0], sz[1] * sz[2], sz[3]).transpose(1, 2).contiguous(), lens)
        plain_ids, plain_strs = model.decoder.beam_search(enc, args, beam_width=SPEC['beam_width'], nbest=SPEC['nbest'],
                                                          start_token=vocab.SOS_ID)

    # the LM: the reference's RNNModel from a seed, its vocabulary projection perturbed (seeded) so that it is far from uniform
    words = ['<oov>', '<eos>'] + lm_words(plain_ids, lambda s: mtl_amd.lm_string(s, vocab))
    n_harvested = len(words) - 2
    words += ['w%03d' % i for i in range(SPEC['lm_ntoken'] - len(words))]
    torch.manual_seed(SPEC['lm_seed'])
    net = ref_lm.RNNModel('LSTM', SPEC['lm_ntoken'], SPEC['lm_ninp'], SPEC['lm_nhid'], SPEC['lm_nlayers'], SPEC['lm_dropout'], False)
    g = torch.Generator().manual_seed(SPEC['lm_noise_seed'])
    with torch.no_grad():
        net.decoder.weight += SPEC['lm_noise'] * torch.randn(net.decoder.weight.shape, generator=g)
        net.decoder.bias += SPEC['lm_noise'] * torch.randn(net.decoder.bias.shape, generator=g)
    h = hashlib.sha256()
    for _, p in net.named_parameters():
        h.update(p.detach().numpy().tobytes())
    ckpt = dict(word2idx={w: i for i, w in enumerate(words)}, idx2word=list(words), ntoken=SPEC['lm_ntoken'], ninp=SPEC['lm_ninp'],
                nhid=SPEC['lm_nhid'], nlayers=SPEC['lm_nlayers'], dropout=SPEC['lm_dropout'], tie_weights=False,
                model_state_dict=net.state_dict())
    path = '/tmp/golden_R0_lm.pt'
    torch.save(ckpt, path)
    lm = ref_lm.LM(path, argparse.Namespace(cuda=False))

    seen = []                                                   # the strings LM.evaluate receives, in call order
    real_eval = ref_lm.LM.evaluate

    def spy_eval(self, seq):
        seen.append(seq)
        return real_eval(self, seq)
    ref_lm.LM.evaluate = spy_eval
    ended_log = []                                              # each utterance's ended hypotheses, in their final sorted order

    def spy_sorted(items, key=None, reverse=False):
        out = sorted(items, key=key, reverse=reverse)
        if items and 'final_score' in items[0] and (not ended_log or ended_log[-1][1] is not items):
            ended_log.append(([(list(map(int, h['yseq'].reshape(-1).tolist())), float(h['score']), float(h['final_score']))
                               for h in out], items))
        return out
    ref_dec.sorted = spy_sorted
    try:
        with torch.no_grad():
            lm_ids, lm_strs = model.decoder.beam_search(enc, args, beam_width=SPEC['beam_width'], nbest=SPEC['nbest'],
                                                        lm_rescoring=True, lm=lm, lm_weight=SPEC['lm_weight'],
                                                        c_weight=SPEC['c_weight'], start_token=vocab.SOS_ID)
            _, eval_strs, _ = model.evaluate(x, lens, y, args, beam_search=True, lm_rescoring=True, lm=lm, lm_weight=SPEC['lm_weight'],
                                             c_weight=SPEC['c_weight'], start_token=vocab.SOS_ID)
    finally:
        del ref_dec.sorted
        ref_lm.LM.evaluate = real_eval
    ended = [e for e, _ in ended_log[:SPEC['k']]]
    assert len(ended) == SPEC['k'] and eval_strs == lm_strs
    n_eval = len(seen) // 2
    seen = seen[:n_eval]
    assert lm_strs[0].strip(), 'the best hypothesis must not be empty (the reference would switch to greedy)'

    # the LM must change the n-best order somewhere; rankings must not hinge on near-ties
    def per_utt(ids):
        out, i = [], 0
        for e in ended:
            n = min(len(e), SPEC['nbest'])
            out.append(ids[i:i + n])
            i += n
        return out
    changed = sum(a != b for a, b in zip(per_utt(lm_ids), per_utt(plain_ids)))
    assert changed >= 1, 'the LM does not change any n-best order'
    gaps = [abs(e[i][2] - e[i + 1][2]) for e in ended for i in range(len(e) - 1)]
    min_gap = min(gaps)
    assert min_gap >= 1e-3, min_gap
    n_oov = sum(sum(w not in ckpt['word2idx'] for w in s.split()) for s in seen)
    assert 0 < n_oov < sum(len(s.split()) for s in seen)

    # calculate_lm_score on hand-made hypotheses: empty, all out-of-vocabulary, mixed scripts, double spaces
    lid = vocab.label2id
    sp = [i for i, c in enumerate(vocab.id2label) if c == ' '][0]
    latin = [lid[c] for c in 'abcdefghij' if c in lid]
    cjk = [i for i, c in enumerate(vocab.id2label) if len(c) == 1 and ord(c) >= 0x4e00][:6]
    hand = [[1, 2], [1, sp, sp, 2], [1] + latin[:3] + [sp] + latin[3:5] + [2], [1] + cjk[:2] + [sp] + latin[:2] + [sp] + cjk[2:4] + [2],
            [1, sp] + latin[:2] + [sp, sp] + cjk[:1] + [sp, sp, sp] + latin[2:3] + [2], [0, 1] + cjk[:3] + [2, 0]]
    hand += [lm_ids[0], lm_ids[-1]]
    hand_out = []
    for yseq in hand:
        import torch as _t
        sc, nw, oov = ref_lm.calculate_lm_score(_t.tensor([yseq]), lm, vocab)
        hand_out.append((float(sc), int(nw), int(oov)))

    def ragged(rows):
        w = max(len(r) for r in rows)
        a = np.full((len(rows), w), -1, dtype=np.int64)
        for i, r in enumerate(rows):
            a[i, :len(r)] = r
        return a
    enc_str = lambda lst: np.frombuffer('\n'.join(lst).encode('utf-8'), dtype=np.uint8)
    flat_ended = [h for e in ended for h in e]
    store = dict(spec=np.frombuffer(json.dumps(SPEC).encode(), dtype=np.uint8),
                 labels=enc_str(labs), lm_words=enc_str(words), lm_sha256=np.frombuffer(h.hexdigest().encode(), dtype=np.uint8),
                 lm_ids=ragged(lm_ids), lm_strs=enc_str(lm_strs), plain_ids=ragged(plain_ids), plain_strs=enc_str(plain_strs),
                 ended_ids=ragged([e[0] for e in flat_ended]), ended_score=np.array([e[1] for e in flat_ended], dtype=np.float32),
                 ended_final=np.array([e[2] for e in flat_ended], dtype=np.float32),
                 ended_count=np.array([len(e) for e in ended], dtype=np.int64),
                 lm_seen=enc_str(seen), hand_ids=ragged(hand), hand_score=np.array([o[0] for o in hand_out], dtype=np.float32),
                 hand_num_words=np.array([o[1] for o in hand_out], dtype=np.int64), hand_oov=np.array([o[2] for o in hand_out], dtype=np.int64),
                 min_gap=np.float32(min_gap))
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'R0.npz'), **store)
    print('R0: %d utterances, %d ended hypotheses (%s), %d LM strings, %d harvested words, %d OOV words, n-best changed in %d, '
          'min gap %.3e' % (len(ended), len(flat_ended), [len(e) for e in ended], len(seen), n_harvested, n_oov, changed, min_gap))
    for s in lm_strs:
        print('   ', repr(s))
    for s, o in zip(hand, hand_out):
        print('   ', repr(mtl_amd.lm_string(s, vocab)), o)


if __name__ == '__main__':
    main()
