"""Tokens per second of LM evaluation on a 35 000-token stream, batch 10, bptt 35, 2-layer LSTM, ntoken 30 011:

  * evaluate : lm.evaluate = LMEngine.evaluate (windows chunked into one recurrent call, fused projection + log-sum-exp, keyed fp64
               sums on the device, one read-back);
  * window_loop : the loop a user had to write before -- RNNModel.forward per window (logits written), torch cross-entropy on the
               returned logits, the carried state, one read-back of the total at the end -- on the same device.

Run at nhid = ninp = 512 (persistent recurrent kernels) and 200 (per-step path).  After one warm-up pass of each, the two paths are
timed in alternation, `--rounds` wall-clock passes each (every pass ends with a host read-back); reported per path: the median tokens/s
and the spread (slowest, fastest).

    python tools/bench_lm_eval.py [--rounds 3] [--out profiles/lm_eval.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(ntoken=30011, nlayers=2, bptt=35, batch=10, tokens=35000, dropout=0.2)


def window_loop(model, source, bptt):
    def run():
        model.eval()
        hidden = model.init_hidden(source.shape[1])
        total = torch.zeros((), device=source.device)
        for i in range(0, source.size(0) - 1, bptt):
            n = min(bptt, source.size(0) - 1 - i)
            out, hidden = model(source[i:i + n], hidden)
            total += n * torch.nn.functional.cross_entropy(out.view(-1, out.size(-1)), source[i + 1:i + 1 + n].reshape(-1))
        return float(total) / source.size(0)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_eval.json'))
    a = ap.parse_args()
    import mtl_amd
    assert torch.cuda.is_available(), 'bench_lm_eval needs an MI355X'
    s = SHAPE
    source = mtl_amd.lm.batchify(mtl_amd.lm.synth_corpus(1, s['ntoken'], s['tokens']), s['batch']).cuda()
    ntok = (source.shape[0] - 1) * source.shape[1]
    res = dict(device=torch.cuda.get_device_name(0), shape=s, rounds=a.rounds, unit='tokens per second', widths={})
    for H in (512, 200):
        torch.manual_seed(0)
        model = mtl_amd.lm.RNNModel('LSTM', s['ntoken'], H, H, s['nlayers'], s['dropout']).cuda()
        paths = {'evaluate': lambda: mtl_amd.lm.evaluate(model, source, s['bptt']), 'window_loop': window_loop(model, source, s['bptt'])}
        loss = {k: fn() for k, fn in paths.items()}                      # warm-up: code objects, buffer pools
        assert abs(loss['evaluate'] - loss['window_loop']) <= 1e-4 * loss['window_loop'], loss
        rate = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rate[k].append(ntok / (time.perf_counter() - t0))
        res['widths'][str(H)] = dict(persistent=bool(model.engine.lib.mtl_lstm_layer_supported(s['batch'], H)), loss=loss,
                                     paths={k: dict(median=round(statistics.median(v)), min=round(min(v)), max=round(max(v)))
                                            for k, v in rate.items()})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
