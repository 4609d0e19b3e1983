"""Milliseconds per window of LM epoch training on the device: one epoch of 200 windows (199 of bptt 35 and a
last one of 7 steps, batch 20) over a lm.synth_corpus stream with ntoken 10000, at two configurations --

  * lstm200 : the reference's default, LSTM 200/200, 2 layers;
  * gru512  : the README's GRU, 512/512, 2 layers --

and these legs, alternated `--rounds` times in one process after one warm-up epoch each (every shape, the short last window included):

  * trainer      : lm.LMTrainer.train_epoch (one mtl_lm_window_chains table per stream, mtl_sumsq + mtl_sgd_clip_step per window);
  * parent       : the same loop composed here from the calls the project had before -- per window g.zero_(), LMEngine.forward /
                   backward with chains from LMEngine._chains, mtl_sumsq, mtl_scale, mtl_axpy, the loss added on the device;
  * parent+table : `parent` with the chains taken from the table (what mtl_lm_window_chains alone buys);
  * parent+step  : `parent` with mtl_sgd_clip_step in place of zero / scale / axpy / loss add (what that kernel alone buys);
  * torch        : torch.nn.LSTM / GRU + Embedding + Linear with autograd, clip_grad_norm_ and torch.optim.SGD on the same device.

Timed with a host clock around an epoch that ends in a device synchronise; reported per leg: the median, the fastest and the slowest
epoch in ms per window.  No loss is read inside an epoch (200 windows never reach a log point at log_interval 200).

    python tools/bench_lm_train.py [--rounds 5] [--out profiles/lm_train.json]
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
NTOKEN, BPTT, BATCH, WINDOWS, LAST, DROPOUT, LR, CLIP = 10000, 35, 20, 200, 7, 0.2, 20.0, 0.25
CONFIGS = {'lstm200': dict(rnn_type='LSTM', ninp=200, nhid=200, nlayers=2), 'gru512': dict(rnn_type='GRU', ninp=512, nhid=512, nlayers=2)}


def composed_epoch(model, stream, table=None, fused=False):
    """the epoch of LMTrainer.train_epoch from the earlier calls; table / fused swap in one of the two new kernels"""
    import mtl_amd
    lib, check = mtl_amd._lib.lib(), mtl_amd._lib.check
    eng, theta = model.engine, model.flat_parameters
    dev, n = theta.device, theta.numel()
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    g = torch.zeros_like(theta)
    coef = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(2048, dtype=torch.float32, device=dev)
    total = torch.zeros(1, dtype=torch.float32, device=dev)
    model.train()
    S, B = int(stream.shape[0]), int(stream.shape[1])
    hidden = model.init_hidden(B)
    for i, T in mtl_amd.lm.window_schedule(S, BPTT):
        if not fused:
            g.zero_()
        out = eng.forward(theta, stream[i:i + T], stream[i + 1:i + 1 + T].reshape(-1), hidden, model.dropout_rate,
                          chains=table[:, i * B:(i + T) * B] if table is not None else None)
        hidden = out['hidden']
        eng.backward(g, 1.0)
        check(lib.mtl_sumsq(st(), g.data_ptr(), n, coef.data_ptr(), ws.data_ptr(), 2, CLIP), 'mtl_sumsq')
        if fused:
            check(lib.mtl_sgd_clip_step(st(), theta.data_ptr(), g.data_ptr(), LR, coef.data_ptr(), n, out['loss'].data_ptr(),
                                        total.data_ptr()), 'mtl_sgd_clip_step')
        else:
            check(lib.mtl_scale(st(), g.data_ptr(), 1.0, coef.data_ptr(), n), 'mtl_scale')
            check(lib.mtl_axpy(st(), theta.data_ptr(), g.data_ptr(), -LR, n), 'mtl_axpy')
            total += out['loss']
    torch.cuda.synchronize(dev)
    eng.check_handoff()


def torch_leg(cfg, stream):
    import mtl_amd
    torch.manual_seed(0)
    enc = torch.nn.Embedding(NTOKEN, cfg['ninp']).cuda()
    rnn = getattr(torch.nn, cfg['rnn_type'])(cfg['ninp'], cfg['nhid'], cfg['nlayers'], dropout=DROPOUT).cuda()
    dec = torch.nn.Linear(cfg['nhid'], NTOKEN).cuda()
    drop = torch.nn.Dropout(DROPOUT)
    params = list(enc.parameters()) + list(rnn.parameters()) + list(dec.parameters())
    opt = torch.optim.SGD(params, lr=LR)
    sched = mtl_amd.lm.window_schedule(stream.shape[0], BPTT)
    lstm = cfg['rnn_type'] == 'LSTM'

    def run():
        h = torch.zeros(cfg['nlayers'], BATCH, cfg['nhid'], device='cuda')
        hidden = (h, h.clone()) if lstm else h
        total = torch.zeros((), device='cuda')
        for i, T in sched:
            hidden = tuple(t.detach() for t in hidden) if lstm else hidden.detach()
            opt.zero_grad()
            out, hidden = rnn(drop(enc(stream[i:i + T])), hidden)
            loss = torch.nn.functional.cross_entropy(dec(drop(out).view(-1, cfg['nhid'])), stream[i + 1:i + 1 + T].reshape(-1))
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, CLIP)
            opt.step()
            total += loss.detach()
        torch.cuda.synchronize()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_train.json'))
    a = ap.parse_args()
    import mtl_amd
    lm = mtl_amd.lm
    assert torch.cuda.is_available(), 'bench_lm_train needs an MI355X'
    S = (WINDOWS - 1) * BPTT + LAST + 1
    stream = lm.batchify(lm.synth_corpus(1, NTOKEN, S * BATCH), BATCH).cuda()
    assert len(lm.window_schedule(S, BPTT)) == WINDOWS and lm.window_schedule(S, BPTT)[-1][1] == LAST
    res = dict(device=torch.cuda.get_device_name(0), windows=WINDOWS, bptt=BPTT, batch=BATCH, ntoken=NTOKEN, dropout=DROPOUT,
               rounds=a.rounds, unit='ms per window (host clock around one epoch ending in a device synchronise)', configs={})
    for name, cfg in CONFIGS.items():
        def make():
            torch.manual_seed(0)
            return lm.RNNModel(cfg['rnn_type'], NTOKEN, cfg['ninp'], cfg['nhid'], cfg['nlayers'], DROPOUT).cuda()
        models = {k: make() for k in ('trainer', 'parent', 'parent+table', 'parent+step')}
        trainer = lm.LMTrainer(models['trainer'], lr=LR, clip=CLIP, bptt=BPTT)
        table = trainer.chain_table(stream, BPTT)
        assert table is not None
        legs = {'trainer': lambda: trainer.train_epoch(stream),
                'parent': lambda: composed_epoch(models['parent'], stream),
                'parent+table': lambda: composed_epoch(models['parent+table'], stream, table=table),
                'parent+step': lambda: composed_epoch(models['parent+step'], stream, fused=True),
                'torch': torch_leg(cfg, stream)}
        for fn in legs.values():                 # warm-up: every window shape of the epoch, code objects, buffer pools
            fn()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1000 / WINDOWS)
        res['configs'][name] = dict(cfg, legs={k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                                               for k, v in times.items()})
        print(name, json.dumps(res['configs'][name]['legs']), flush=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
