"""Test-set evaluation: the reference's test.py:112-171 `evaluate` loop (CER, WER and the per-language CER over a test loader); the
hypotheses come from Transformer.evaluate, i.e. the searches of decode.py."""
import time

import torch

from .functions import post_process
from .metrics import calculate_cer, calculate_cer_en_zh, calculate_wer

TOTALS = ('total_word', 'total_char', 'total_cer', 'total_wer', 'total_en_cer', 'total_zh_cer', 'total_en_char', 'total_zh_char',
          'total_hyp_char', 'total_time')
LINE = 'TEST CER:{:.2f}% WER:{:.2f}% CER_EN:{:.2f}% CER_ZH:{:.2f}% TOTAL_TIME:{:.7f} TOTAL HYP CHAR:{:.2f}'


def evaluate_test_set(model, vocab, test_loader, args, lm=None, start_token=-1, device_ranking=True, on_batch=None):
    """test.py:112-171.  Per batch of `test_loader` ((src, trg, src_percentages, src_lengths, trg_lengths), as AudioDataLoader
    yields them): model.evaluate with the reference's keyword set (args.lm_rescoring, lm_weight, beam_search, beam_width,
    beam_nbest, c_weight, verbose), post_process on hypothesis and gold strings, calculate_wer(hyp, gold),
    calculate_cer(hyp.strip(), gold.strip()), calculate_cer_en_zh(hyp, gold); the totals are accumulated over the test set and the
    reference's `TEST CER:... WER:... CER_EN:... CER_ZH:... TOTAL_TIME:... TOTAL HYP CHAR:...` line is printed after every batch.

    Like the reference, hypothesis x of the batch's concatenated n-best list is compared with gold string x.  That pairs every
    utterance with its own best hypothesis only for args.beam_nbest == 1 or batches of one utterance (model.evaluate returns ALL
    n-best strings of all utterances in a row); kept as it is, because the reference's published numbers are computed this way.

    device_ranking: beam search through PassEngine.beam_decode_batch (hypotheses ranked on the device); ignored by the greedy
    search.  on_batch(totals): optional callback with a copy of the running totals after every batch.
    -> dict of the totals, time_per_word, the four percentages (cer, wer, cer_en, cer_zh) and the last printed line."""
    model.eval()
    t = dict.fromkeys(TOTALS, 0)
    line = None
    on_device = next(model.parameters()).is_cuda
    with torch.no_grad():
        for data in test_loader:
            src, trg, _src_percentages, src_lengths, _trg_lengths = data
            if on_device:
                src, trg = src.cuda(), trg.cuda()
            start_time = time.time()
            _ids, batch_strs_hyps, batch_strs_gold = model.evaluate(
                src, src_lengths, trg, args, lm_rescoring=args.lm_rescoring, lm=lm, lm_weight=args.lm_weight, beam_search=args.beam_search,
                beam_width=args.beam_width, beam_nbest=args.beam_nbest, c_weight=args.c_weight, start_token=start_token,
                verbose=args.verbose, device_ranking=device_ranking)
            for x in range(len(batch_strs_gold)):
                hyp = post_process(batch_strs_hyps[x], vocab.special_token_list)
                gold = post_process(batch_strs_gold[x], vocab.special_token_list)
                wer = calculate_wer(hyp, gold)
                cer = calculate_cer(hyp.strip(), gold.strip())
                if args.verbose:
                    print('HYP', hyp)
                    print('GOLD:', gold)
                    print('CER:', cer)
                en_cer, zh_cer, num_en_char, num_zh_char = calculate_cer_en_zh(hyp, gold)
                t['total_en_cer'] += en_cer
                t['total_zh_cer'] += zh_cer
                t['total_en_char'] += num_en_char
                t['total_zh_char'] += num_zh_char
                t['total_hyp_char'] += len(hyp)
                t['total_wer'] += wer
                t['total_cer'] += cer
                t['total_word'] += len(gold.split(' '))
                t['total_char'] += len(gold)
            t['total_time'] += time.time() - start_time
            line = LINE.format(*_rates(t), t['total_time'], t['total_hyp_char'])
            print(line, flush=True)
            if on_batch is not None:
                on_batch(dict(t))
    out = dict(t)
    if line is not None:
        out['cer'], out['wer'], out['cer_en'], out['cer_zh'] = _rates(t)
        out['time_per_word'] = t['total_time'] / t['total_word']
    out['line'] = line
    return out


def _rates(t):
    return (t['total_cer'] * 100 / t['total_char'], t['total_wer'] * 100 / t['total_word'],
            t['total_en_cer'] * 100 / max(1, t['total_en_char']), t['total_zh_cer'] * 100 / max(1, t['total_zh_char']))
