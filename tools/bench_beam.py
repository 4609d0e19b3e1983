"""Utterances per second of the host-ranked beam search (PassEngine.beam_decode, one utterance at a time, logits read back at every
position) and of the device-ranked one (PassEngine.beam_decode_batch: mtl_beam_rank + mtl_beam_gather, a chunk of utterances per decoder
step), DESIGN.md "Test-set evaluation".  Same process, same parameters, same encoder memories: the F0-size model at its initial
parameters (no hypothesis ends before the forced EOS: the longest searches) and with the B0 perturbation of the vocabulary projection
(hypotheses end early), W = 5, nbest = 5.  After a warm-up that lets both paths record their command lists, each search runs
`--reps` times, interleaved.  The two n-best lists are compared on the way.

    python tools/bench_beam.py [--reps 3] [--utterances 12] [--frames 128]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--utterances', type=int, default=12)
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--beam-width', type=int, default=5)
    ap.add_argument('--nbest', type=int, default=5)
    a = ap.parse_args()
    import mtl_amd
    from oracle import refimpl as R
    from tests import golden_util as gu
    z, cfg, spec = gu.load('F0')
    bspec = gu.load_beam()[0]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), model='F0', W=a.beam_width, nbest=a.nbest, utterances=a.utterances,
                          frames=a.frames)))
    for params in ('init', 'B0-perturbed'):
        margs = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
                                   dropout=0.0, emb_trg_sharing=False, label_smoothing=0.0, name='bench_beam', cuda=True,
                                   **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
        vocab = mtl_amd.synthetic_vocab(cfg['vocab_size'])
        torch.manual_seed(123456)
        model = mtl_amd.init_transformer_model(margs, vocab, r=cfg['r'])
        if params != 'init':
            gu.perturb_output_layer(model.decoder.output_linear.weight, bspec)
        model = model.cuda()
        model.eval()
        eng = model.engine
        x, lens, y = R.synth_batch(4242, a.utterances, a.frames, 8, cfg['vocab_size'], True)
        eng.widen = '0'
        model.pass_forward(x.cuda(), lens, y)
        mem = eng.arena['e%d.ff.y' % (eng.hp.n_enc - 1)].clone()
        T4, k, W = (a.frames // 2) // 2, a.utterances, a.beam_width
        theta, nw = model.flat_parameters, model._num_words
        tgt = cfg['tgt_max_len']

        def host():
            return [eng.beam_decode(theta, mem.data_ptr() + 4 * b * T4 * eng.hp.d, T4, vocab.SOS_ID, W, a.nbest, tgt, nw, vocab.EOS_ID, 1.0)
                    for b in range(k)]

        def device():
            return eng.beam_decode_batch(theta, mem.data_ptr(), k, T4, vocab.SOS_ID, W, a.nbest, tgt, nw, vocab.EOS_ID, 1.0)
        for _ in range(3):                                    # eager, recording, first replay
            h, d = host(), device()
        same_ids = [[s for s, _ in u] for u in h] == [[s for s, _ in u] for u in d]
        times = dict(host=[], device=[])
        for _ in range(a.reps):
            for name, fn in (('host', host), ('device', device)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(k / (time.perf_counter() - t0))
        lists = eng.replay_beam_batch.recorded()
        per_pos = max(cl.n for cl in lists) / eng.BEAM_POLL if lists else None
        positions = [max(len(s) for s, _ in u) - 1 if u else 0 for u in d]
        print(json.dumps(dict(params=params, host_utt_per_s=[round(v, 2) for v in times['host']],
                              device_utt_per_s=[round(v, 2) for v in times['device']],
                              ratio_slowest_device_over_fastest_host=round(min(times['device']) / max(times['host']), 3),
                              spreads_overlap=bool(min(times['device']) <= max(times['host'])), same_ids=same_ids,
                              chunk=eng.beam_chunk(W), poll_every=eng.BEAM_POLL, library_calls_per_position=per_pos, T4=T4,
                              longest_hypothesis=max(positions))), flush=True)


if __name__ == '__main__':
    main()
