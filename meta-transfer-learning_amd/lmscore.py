"""LM rescoring of finished beam hypotheses: drop-ins for `utils/lm.py` of the reference (`LM`, `calculate_lm_score`) and the
batched form the accelerated beam search uses (`lm_string`, `rescore`).

The word-level LSTM LM runs on the device (lm.RNNModel / LMEngine.sequence_nll: one ragged batch, one fused vocabulary projection
+ log-sum-exp).  Rescoring only ORDERS the ended hypotheses of an utterance (modules/decoder.py:248-264, 280-281: `final_score`
never takes part in pruning), so scoring all of them after the search, in one batch, gives the reference's result.
"""
import math

import numpy as np
import torch

from .data import is_contain_chinese_word, get_word_segments_per_language
from .lm import RNNModel

EMPTY = (-999, 0, 0)          # calculate_lm_score of a hypothesis without words (utils/lm.py:33-34)


class LM(object):
    """utils/lm.py:42-155: a `torch.load` checkpoint dict with word2idx, idx2word, ntoken, ninp, nhid, nlayers, dropout,
    tie_weights and model_state_dict (the parameter names of lm.RNNModel)."""

    def __init__(self, model_path, args=None):
        self.model_path = model_path
        checkpoint = torch.load(model_path, map_location='cpu', weights_only=False)
        self.word2idx, self.idx2word = checkpoint['word2idx'], checkpoint['idx2word']
        if checkpoint.get('rnn_type', 'LSTM') != 'LSTM':
            raise NotImplementedError('LM rescoring: only LSTM language models are accelerated (checkpoint rnn_type=%r)'
                                      % checkpoint['rnn_type'])
        if checkpoint['tie_weights']:
            raise NotImplementedError('LM rescoring: checkpoints with tie_weights=True are not supported (the accelerated LM keeps '
                                      'decoder.weight separate from encoder.weight)')
        self.model = RNNModel('LSTM', ntoken=checkpoint['ntoken'], ninp=checkpoint['ninp'], nhid=checkpoint['nhid'],
                              nlayers=checkpoint['nlayers'], dropout=checkpoint['dropout'], tie_weights=False)
        self.model.load_state_dict(checkpoint['model_state_dict'])
        self.model.eval()
        self.cuda = bool(getattr(args, 'cuda', True)) and torch.cuda.is_available()
        if self.cuda:
            self.model = self.model.cuda()

    def seq_to_tensor(self, seq):
        """utils/lm.py:87-102 -> (ids (n + 1,) int64 over seq.split() + ['<eos>'], number of out-of-vocabulary words)"""
        words = seq.split() + ['<eos>']
        oov_id = self.word2idx['<oov>']
        ids = [self.word2idx.get(w, oov_id) for w in words]
        return torch.tensor(ids, dtype=torch.int64), sum(w not in self.word2idx for w in words)

    def score(self, seqs):
        """LM.evaluate of every string in `seqs`, in ONE batched device pass -> (total_loss (N,) fp32 numpy, [oov counts]).
        total_loss = n * mean cross-entropy of the n next-word predictions (the first word is never predicted), in the reference's
        fp32 order; NaN for a string without words (the reference's loss over an empty batch)."""
        enc = [self.seq_to_tensor(s) for s in seqs]
        if not enc:
            return np.zeros(0, dtype=np.float32), []
        n = [int(ids.numel()) - 1 for ids, _ in enc]
        T = max(max(n), 1)
        ids = torch.zeros(T, len(enc), dtype=torch.int64)
        tgt = torch.full((T, len(enc)), -1, dtype=torch.int64)
        for b, (t, _) in enumerate(enc):
            ids[:n[b], b] = t[:n[b]]
            tgt[:n[b], b] = t[1:]
        eng = self.model._need_engine()
        nll = eng.sequence_nll(self.model.flat_parameters, ids, tgt).cpu().numpy()
        total = np.full(len(enc), np.nan, dtype=np.float32)
        for b, k in enumerate(n):
            if k > 0:
                total[b] = np.float32(k) * (nll[b] / np.float32(k))       # len(data) * CrossEntropyLoss() (mean) of :131-133
        return total, [o for _, o in enc]

    def evaluate(self, seq):
        """utils/lm.py:112-136 -> (total_loss 0-dim fp32 tensor, oov_token)"""
        total, oov = self.score([seq])
        return torch.tensor(total[0]), oov[0]


def lm_string(seq, vocab):
    """utils/lm.py:12-30: the string calculate_lm_score hands to LM.evaluate ('' when the hypothesis has no words).
    seq: the reference's (1, L) tensor, a 1-D tensor or a list of ids."""
    if torch.is_tensor(seq):
        seq = seq.reshape(-1).tolist()
    seq_str = ''.join(vocab.id2label[int(c)] for c in seq).replace(vocab.PAD_TOKEN, '').replace(vocab.SOS_TOKEN, '').replace(vocab.EOS_TOKEN, '')
    seq_str = seq_str.replace('  ', ' ')
    out = ''
    for seg in get_word_segments_per_language(seq_str):
        if is_contain_chinese_word(seg):
            for char in seg:
                if out != '':
                    out += ' '
                out += char
        else:
            if out != '':
                out += ' '
            out += seg
    return out.replace('  ', ' ').replace('  ', ' ')


def calculate_lm_score(seq, lm, vocab):
    """utils/lm.py:8-37 -> (lm_score, num_words, oov): (-total_loss / n + 1, n + 1, oov) over the n words of lm_string(seq),
    (-999, 0, 0) without words"""
    seq_str = lm_string(seq, vocab)
    if seq_str == '':
        return EMPTY
    score, oov_token = lm.evaluate(seq_str)
    return -1 * score / len(seq_str.split()) + 1, len(seq_str.split()) + 1, oov_token


def rescore(hyps, lm, vocab, lm_weight, c_weight):
    """modules/decoder.py:251-256 for a list of ended hypotheses (dicts with 'score' (fp32) and 'yseq'), all scored in ONE
    LM.score batch: sets 'lm_score', 'num_words' and 'final_score' on each, in the reference's fp32 arithmetic."""
    strs = [lm_string(h['yseq'], vocab) for h in hyps]
    todo = [i for i, s in enumerate(strs) if s != '']
    total, oov = lm.score([strs[i] for i in todo])
    f32 = np.float32
    res = {i: (total[j], oov[j]) for j, i in enumerate(todo)}
    for i, h in enumerate(hyps):
        if i in res:
            n = len(strs[i].split())
            lm_score = f32(f32(-res[i][0]) / f32(n)) + f32(1)           # -1 * score / n + 1
            lm_score = f32(lm_score - f32(res[i][1] * 2))                # lm_score -= oov_token * 2
            num_words = n + 1
            h['final_score'] = f32(f32(h['score'] + f32(f32(lm_weight) * lm_score)) + f32(math.sqrt(num_words) * c_weight))
        else:
            lm_score, num_words = EMPTY[0], EMPTY[1]                     # python numbers: lm_weight * -999 in double
            h['final_score'] = f32(f32(h['score'] + f32(lm_weight * lm_score)) + f32(math.sqrt(num_words) * c_weight))
        h['lm_score'], h['num_words'] = lm_score, num_words
    return hyps
