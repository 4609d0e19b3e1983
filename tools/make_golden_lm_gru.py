"""Generate tests/golden/LG0.npz: the REAL reference `lm/model/rnn_model.py:RNNModel` for `--model GRU` and `--tied`.

Runs only where the reference checkout exists (it imports the reference's own module, as oracle/make_golden.py does for L0, and
copies nothing).  For a GRU untied, a GRU tied and an LSTM tied model at a small spec it records the sha256 of the initial
parameters, the `named_parameters()` and `state_dict()` key lists, and the logits + new hidden state of one eval-mode (T = 7, B = 3)
batch from a non-zero carried state.

    python tools/make_golden_lm_gru.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = dict(seed=1234, ntoken=300, nlayers=2, T=7, B=3, data_seed=9,
            models=dict(gru=dict(rnn_type='GRU', ninp=48, nhid=64, tied=False), gru_tied=dict(rnn_type='GRU', ninp=64, nhid=64, tied=True),
                        lstm_tied=dict(rnn_type='LSTM', ninp=64, nhid=64, tied=True)))


def main():
    sys.path.insert(0, '/root/reference/lm')
    import torch
    from model.rnn_model import RNNModel
    torch.set_num_threads(8)
    store = {'spec': np.frombuffer(json.dumps(SPEC).encode(), dtype=np.uint8)}
    g = torch.Generator().manual_seed(SPEC['data_seed'])
    x = torch.randint(0, SPEC['ntoken'], (SPEC['T'], SPEC['B']), generator=g)
    store['x'] = x.numpy()
    for key, ms in SPEC['models'].items():
        torch.manual_seed(SPEC['seed'])
        model = RNNModel(ms['rnn_type'], SPEC['ntoken'], ms['ninp'], ms['nhid'], SPEC['nlayers'], 0.5, ms['tied'])
        model.eval()
        h = hashlib.sha256()
        for _, p in model.named_parameters():
            h.update(p.detach().numpy().tobytes())
        store[key + '/theta0_sha256'] = np.frombuffer(h.hexdigest().encode(), dtype=np.uint8)
        store[key + '/param_names'] = np.array([n for n, _ in model.named_parameters()])
        store[key + '/state_keys'] = np.array(list(model.state_dict().keys()))
        hidden = model.init_hidden(SPEC['B'])
        lstm = isinstance(hidden, tuple)
        hidden = tuple(0.3 * torch.randn(t.shape, generator=g) for t in hidden) if lstm else 0.3 * torch.randn(hidden.shape, generator=g)
        with torch.no_grad():
            out, hn = model(x, hidden)
        for i, (a, b) in enumerate(zip(hidden if lstm else (hidden,), hn if lstm else (hn,))):
            store['%s/h0_%d' % (key, i)], store['%s/hn_%d' % (key, i)] = a.numpy(), b.numpy()
        store[key + '/out'] = out.numpy()
        print('%-10s %d parameters, %d state keys, |out| %.4f' % (key, len(store[key + '/param_names']), len(store[key + '/state_keys']),
                                                                float(out.norm())))
    path = os.path.join(ROOT, 'tests', 'golden', 'LG0.npz')
    np.savez_compressed(path, **store)
    print('LG0 written: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
