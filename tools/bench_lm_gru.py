"""Forward + backward time of the GRU language model at the bench LM shapes (ntoken 10000, ninp = nhid = 512, 2 layers, bptt 35,
batch 20, dropout 0.2) on the device:

  * gru_persistent : lm.RNNModel('GRU'), one persistent launch per layer and direction (csrc/mtl_gru.hip);
  * gru_steps      : the same model with LMEngine.persistent = False (recurrent product + cell kernel per step);
  * torch_gru      : torch.nn.GRU + nn.Linear + cross-entropy with autograd on the same device -- what a user would run otherwise;
  * lstm_layers    : lm.RNNModel('LSTM') with one launch per layer and direction (LMEngine.stacked = False), for context.

The paths are timed in alternation: `--rounds` rounds, in each round every path runs one span of `--reps` passes between two device
events; reported per path: the median span (ms per pass), the fastest and the slowest (the spread).

    python tools/bench_lm_gru.py [--reps 20] [--rounds 9] [--out profiles/lm_gru.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(ntoken=10000, ninp=512, nhid=512, nlayers=2, bptt=35, batch=20, dropout=0.2)


def product_pass(model, x, y, persistent, stacked):
    eng = model.engine
    hidden = model.init_hidden(x.shape[1])
    grad = torch.zeros_like(model.flat_grad)

    def run():
        eng.persistent, eng.stacked = persistent, stacked
        eng.forward(model.flat_parameters, x, y, hidden, SHAPE['dropout'])
        eng.backward(grad, 1.0)
    return run


def torch_pass(x, y):
    s = SHAPE
    torch.manual_seed(0)
    enc = torch.nn.Embedding(s['ntoken'], s['ninp']).cuda()
    rnn = torch.nn.GRU(s['ninp'], s['nhid'], s['nlayers'], dropout=s['dropout']).cuda()
    dec = torch.nn.Linear(s['nhid'], s['ntoken']).cuda()
    drop = torch.nn.Dropout(s['dropout'])
    params = list(enc.parameters()) + list(rnn.parameters()) + list(dec.parameters())
    h0 = torch.zeros(s['nlayers'], s['batch'], s['nhid'], device='cuda')

    def run():
        for p in params:
            p.grad = None
        out, _ = rnn(drop(enc(x)), h0)
        loss = torch.nn.functional.cross_entropy(dec(drop(out).view(-1, s['nhid'])), y)
        loss.backward()
    return run


def span(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_gru.json'))
    a = ap.parse_args()
    import mtl_amd
    assert torch.cuda.is_available(), 'bench_lm_gru needs an MI355X'
    s = SHAPE
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, s['ntoken'], (s['bptt'], s['batch']), generator=g).cuda()
    y = torch.randint(0, s['ntoken'], (s['bptt'] * s['batch'],), generator=g).cuda()
    torch.manual_seed(0)
    gru = mtl_amd.lm.RNNModel('GRU', s['ntoken'], s['ninp'], s['nhid'], s['nlayers'], s['dropout']).cuda()
    lstm = mtl_amd.lm.RNNModel('LSTM', s['ntoken'], s['ninp'], s['nhid'], s['nlayers'], s['dropout']).cuda()
    assert gru.engine.lib.mtl_gru_layer_supported(s['batch'], s['nhid']) == 1
    paths = {'gru_persistent': product_pass(gru, x, y, True, True), 'gru_steps': product_pass(gru, x, y, False, True),
             'torch_gru': torch_pass(x, y), 'lstm_layers': product_pass(lstm, x, y, True, False)}
    for fn in paths.values():                # warm-up: code objects, buffer pools, library algorithm choices
        span(fn, 5)
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(span(fn, a.reps))
    gru.engine.check_handoff()
    lstm.engine.check_handoff()
    res = dict(device=torch.cuda.get_device_name(0), shape=s, reps=a.reps, rounds=a.rounds, unit='ms per forward + backward pass',
               paths={k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in times.items()})
    med = {k: v['median'] for k, v in res['paths'].items()}
    res['persistent_vs_steps'] = round(med['gru_steps'] / med['gru_persistent'], 3)
    res['persistent_vs_torch'] = round(med['torch_gru'] / med['gru_persistent'], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
