"""Helpers of the LM-rescoring tests: read tests/golden/R0.npz and rebuild its vocabulary and LM checkpoint."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_r0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'R0.npz'))
    dec = lambda k: bytes(z[k]).decode('utf-8').split('\n')
    rows = lambda k: [[int(v) for v in r if v >= 0] for r in z[k]]
    return dict(spec=json.loads(bytes(z['spec']).decode()), labels=dec('labels'), words=dec('lm_words'),
                lm_sha256=bytes(z['lm_sha256']).decode(), lm_ids=rows('lm_ids'), lm_strs=dec('lm_strs'), plain_ids=rows('plain_ids'),
                ended_ids=rows('ended_ids'), ended_score=z['ended_score'], ended_final=z['ended_final'],
                ended_count=[int(v) for v in z['ended_count']], lm_seen=dec('lm_seen'), hand_ids=rows('hand_ids'),
                hand_score=z['hand_score'], hand_num_words=z['hand_num_words'], hand_oov=z['hand_oov'], min_gap=float(z['min_gap']))


def r0_vocab(r0):
    import mtl_amd
    vocab = mtl_amd.Vocab()
    for c in r0['labels']:
        vocab.add_token(c)
        vocab.add_label(c)
    return vocab


def r0_checkpoint(r0, path, **override):
    """the fixture's LM (the reference's RNNModel drawn from the recorded seed, its projection perturbed) saved as the reference's
    checkpoint dict -> (path, sha256 of the parameters)"""
    import hashlib
    from mtl_amd import lm
    s = r0['spec']
    torch.manual_seed(s['lm_seed'])
    net = lm.RNNModel('LSTM', s['lm_ntoken'], s['lm_ninp'], s['lm_nhid'], s['lm_nlayers'], s['lm_dropout'])
    g = torch.Generator().manual_seed(s['lm_noise_seed'])
    with torch.no_grad():
        net.decoder.weight += s['lm_noise'] * torch.randn(net.decoder.weight.shape, generator=g)
        net.decoder.bias += s['lm_noise'] * torch.randn(net.decoder.bias.shape, generator=g)
    h = hashlib.sha256()
    for _, p in net.named_parameters():
        h.update(p.detach().numpy().tobytes())
    words = r0['words']
    ckpt = dict(word2idx={w: i for i, w in enumerate(words)}, idx2word=list(words), ntoken=s['lm_ntoken'], ninp=s['lm_ninp'],
                nhid=s['lm_nhid'], nlayers=s['lm_nlayers'], dropout=s['lm_dropout'], tie_weights=False,
                model_state_dict={k: v.clone() for k, v in net.state_dict().items()})
    ckpt.update(override)
    torch.save(ckpt, path)
    return path, h.hexdigest()
