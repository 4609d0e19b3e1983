"""Generate tests/golden/LT0.npz: the REAL reference `lm/model/rnn_model.py:RNNModel` driven through the epoch loop of lm/main.py and
the joint loop of lm/main_joint.py.

Runs only where the reference checkout exists (it imports the reference's own module, as tools/make_golden_lm_gru.py does, and copies
nothing).  For an LSTM and a GRU model at a small spec (dropout 0):

* epoch: one epoch over a batchified (S = 32, B = 4) stream with bptt = 6 -- five windows of 6 steps and one of 1 -- in the order of
  lm/main.py:256-277: repackage_hidden, model.zero_grad(), forward, nn.CrossEntropyLoss, backward, clip_grad_norm_, a fresh
  torch.optim.SGD(lr).step().  Recorded: the parameters before the epoch and after every window, every window's loss, the final hidden
  state.
* joint: two iterations of three tasks in the order of lm/main_joint.py:290-336: per task forward_one_batch (repackage_hidden,
  model.zero_grad(), forward), the loss weighted (1 - ratio) / 2, (1 - ratio) / 2, ratio, backward; then clip_grad_norm_ and
  SGD.step().  ONE hidden state threads through all tasks and both iterations.  Task i's batch of iteration `it` is the window of its
  stream at offset it * bptt.  Recorded: the parameters before and after every iteration, the unweighted task losses, the final hidden
  state.

    python tools/make_golden_lm_train.py <checkout of the reference>
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = dict(seed=4321, data_seed=17, ntoken=50, ninp=16, nhid=16, nlayers=2, dropout=0.0, lr=2.0, clip=0.25, ratio=0.8, S=32, B=4, bptt=6,
            tasks=3, iterations=2, models=['LSTM', 'GRU'])


def main():
    if len(sys.argv) != 2:
        sys.exit('usage: python tools/make_golden_lm_train.py <checkout of the reference>')
    sys.path.insert(0, os.path.join(sys.argv[1], 'lm'))
    import torch
    import torch.nn as nn
    import torch.optim as optim
    from model.rnn_model import RNNModel
    torch.set_num_threads(1)
    sp = SPEC
    g = torch.Generator().manual_seed(sp['data_seed'])
    stream = torch.randint(0, sp['ntoken'], (sp['S'], sp['B']), generator=g)
    joint = torch.randint(0, sp['ntoken'], (sp['tasks'], sp['S'], sp['B']), generator=g)
    store = {'spec': np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8), 'stream': stream.numpy(), 'joint_streams': joint.numpy()}
    criterion = nn.CrossEntropyLoss()

    def repackage(h):
        return h.detach() if isinstance(h, torch.Tensor) else tuple(repackage(v) for v in h)

    def flat(model):
        return np.concatenate([p.detach().numpy().reshape(-1) for _, p in model.named_parameters()])

    def hid(h):
        return np.stack([t.detach().numpy() for t in (h if isinstance(h, tuple) else (h,))])

    def batch(source, i):
        T = min(sp['bptt'], len(source) - 1 - i)
        return source[i:i + T], source[i + 1:i + 1 + T].reshape(-1)

    for kind in sp['models']:
        torch.manual_seed(sp['seed'])
        model = RNNModel(kind, sp['ntoken'], sp['ninp'], sp['nhid'], sp['nlayers'], sp['dropout'], False)
        store[kind + '/param_names'] = np.array([n for n, _ in model.named_parameters()])
        init = {k: v.clone() for k, v in model.state_dict().items()}
        # ---- lm/main.py:244-277
        model.train()
        hidden = model.init_hidden(sp['B'])
        thetas, losses = [flat(model)], []
        for i in range(0, stream.size(0) - 1, sp['bptt']):
            data, targets = batch(stream, i)
            hidden = repackage(hidden)
            model.zero_grad()
            output, hidden = model(data, hidden)
            loss = criterion(output.view(-1, sp['ntoken']), targets)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), sp['clip'])
            optim.SGD(model.parameters(), lr=sp['lr']).step()
            losses.append(float(loss.data))
            thetas.append(flat(model))
        store[kind + '/epoch_theta'], store[kind + '/epoch_loss'] = np.stack(thetas), np.array(losses, dtype=np.float32)
        store[kind + '/epoch_hidden'] = hid(hidden)
        # ---- lm/main_joint.py:275-336
        model.load_state_dict(init)
        model.train()
        hidden = model.init_hidden(sp['B'])
        thetas, losses = [flat(model)], []
        for it in range(sp['iterations']):
            outer = optim.SGD(model.parameters(), lr=sp['lr'])
            row = []
            for i in range(sp['tasks']):
                x, y = batch(joint[i], it * sp['bptt'])
                hidden = repackage(hidden)                   # forward_one_batch
                model.zero_grad()
                output, hidden = model(x, hidden)
                tr_loss = criterion(output.view(-1, sp['ntoken']), y)
                row.append(float(tr_loss.data))
                tr_loss = tr_loss * (1 - sp['ratio']) / 2 if i < 2 else tr_loss * sp['ratio']
                tr_loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), sp['clip'])
            outer.step()
            losses.append(row)
            thetas.append(flat(model))
        store[kind + '/joint_theta'], store[kind + '/joint_loss'] = np.stack(thetas), np.array(losses, dtype=np.float32)
        store[kind + '/joint_hidden'] = hid(hidden)
        print('%-5s %d parameters; epoch losses %s; joint losses %s' % (kind, thetas[0].size, np.round(store[kind + '/epoch_loss'], 4),
                                                                       np.round(store[kind + '/joint_loss'], 4).tolist()))
    path = os.path.join(ROOT, 'tests', 'golden', 'LT0.npz')
    np.savez_compressed(path, **store)
    print('LT0 written: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
