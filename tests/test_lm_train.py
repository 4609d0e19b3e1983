"""CPU: the LM epoch / joint loops and the checkpoint loader without a GPU.  tests/lm_train_util.py's restatement of lm/main.py's and
lm/main_joint.py's loops against the REAL reference (tests/golden/LT0.npz, tools/make_golden_lm_train.py), the as-written reading of
the joint step, the window schedule, save_lm_checkpoint -> load_lm_checkpoint, and the refusal under several ranks."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import gru_ref as GR
from tests import lm_train_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lt0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'LT0.npz'))
    return z, json.loads(bytes(z['spec']).decode())


def _rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def _model(sp, kind, theta, dtype=torch.float32):
    m = GR.RNNModel(kind, sp['ntoken'], sp['ninp'], sp['nhid'], sp['nlayers'], sp['dropout']).to(dtype)
    U.load_flat(m, torch.from_numpy(theta))
    return m


@pytest.mark.parametrize('kind', ['LSTM', 'GRU'])
def test_restatement_reproduces_the_reference_epoch(lt0, kind):
    """fp32 restatement vs lm/main.py's loop on the reference's own RNNModel: every window's loss and the parameters after every
    window within 1e-6 relative (per window: |loss - want| / want, |theta - want| / |want|), the final hidden state likewise"""
    z, sp = lt0
    torch.set_num_threads(1)
    model = _model(sp, kind, z[kind + '/epoch_theta'][0])
    assert [n for n, _ in model.named_parameters()] == list(z[kind + '/param_names'])
    want_theta, worst = torch.from_numpy(z[kind + '/epoch_theta']), [0.0]

    def after(w):
        worst[0] = max(worst[0], _rel(U.flat(model), want_theta[w + 1]))
    losses, hidden = U.epoch(model, torch.from_numpy(z['stream']), sp['bptt'], sp['lr'], sp['clip'], after)
    assert len(losses) == 6
    e_l = max(abs(float(a) - float(b)) / float(b) for a, b in zip(losses, z[kind + '/epoch_loss']))
    hid = torch.stack(list(hidden) if isinstance(hidden, tuple) else [hidden])
    e_h = _rel(hid, torch.from_numpy(z[kind + '/epoch_hidden']))
    print('LT0 %s epoch: loss %.2e theta %.2e hidden %.2e' % (kind, e_l, worst[0], e_h))
    assert e_l < 1e-6 and worst[0] < 1e-6 and e_h < 1e-6


@pytest.mark.parametrize('kind', ['LSTM', 'GRU'])
def test_restatement_reproduces_the_reference_joint_loop(lt0, kind):
    """the as-written joint iteration vs lm/main_joint.py's loop (two iterations of three tasks, one hidden state through all)"""
    z, sp = lt0
    torch.set_num_threads(1)
    model = _model(sp, kind, z[kind + '/joint_theta'][0])
    streams = torch.from_numpy(z['joint_streams'])
    hidden = model.init_hidden(sp['B'])
    for it in range(sp['iterations']):
        batches = [U.get_batch(streams[i], it * sp['bptt'], sp['bptt']) for i in range(sp['tasks'])]
        _, losses, hidden = U.joint_iteration(model, hidden, batches, sp['lr'], sp['clip'], sp['ratio'], True)
        for a, b in zip(losses, z[kind + '/joint_loss'][it]):
            assert abs(float(a) - float(b)) < 1e-6 * float(b)
        assert _rel(U.flat(model), torch.from_numpy(z[kind + '/joint_theta'][it + 1])) < 1e-6
    hid = torch.stack(list(hidden) if isinstance(hidden, tuple) else [hidden])
    assert _rel(hid, torch.from_numpy(z[kind + '/joint_hidden'])) < 1e-6


def test_as_written_joint_step_is_the_last_tasks_gradient_alone(lt0):
    """model.zero_grad() before every forward: the parameters after an iteration equal ONE step on w_last * g_last taken from the
    hidden state the first two forwards left; accumulating all three weighted gradients gives something else"""
    z, sp = lt0
    streams = torch.from_numpy(z['joint_streams'])
    batches = [U.get_batch(streams[i], 0, sp['bptt']) for i in range(3)]
    theta0 = z['GRU/joint_theta'][0]
    a, b, c = (_model(sp, 'GRU', theta0, torch.float64) for _ in range(3))
    U.joint_iteration(a, a.init_hidden(sp['B']), batches, sp['lr'], sp['clip'], sp['ratio'], True)
    U.joint_iteration(b, b.init_hidden(sp['B']), batches, sp['lr'], sp['clip'], sp['ratio'], False)
    hidden = c.init_hidden(sp['B'])
    with torch.no_grad():
        for x, _ in batches[:2]:
            _, hidden = c(x, hidden)
    params = list(c.parameters())
    out, _ = c(batches[2][0], hidden)
    loss = torch.nn.functional.cross_entropy(out.view(-1, out.size(2)), batches[2][1]) * sp['ratio']
    U.sgd_(params, torch.autograd.grad(loss, params), sp['lr'], sp['clip'])
    assert _rel(U.flat(a), U.flat(c)) < 1e-12
    step = float((U.flat(a) - torch.from_numpy(theta0)).norm())
    assert float((U.flat(b) - U.flat(a)).norm()) > 1e-2 * step


@pytest.mark.parametrize('S,bptt,want', [(32, 6, [(0, 6), (6, 6), (12, 6), (18, 6), (24, 6), (30, 1)]),
                                         (33, 6, [(0, 6), (6, 6), (12, 6), (18, 6), (24, 6), (30, 2)]),
                                         (6, 35, [(0, 5)]), (2, 1, [(0, 1)])])
def test_window_schedule(S, bptt, want):
    import mtl_amd
    assert mtl_amd.lm.window_schedule(S, bptt) == want == U.schedule(S, bptt)
    assert sum(T for _, T in want) == S - 1
    with pytest.raises(ValueError):
        mtl_amd.lm.window_schedule(1, bptt)


def _dictionary(n):
    import mtl_amd
    d = mtl_amd.lm.Dictionary()
    for i in range(n):
        d.add_word('<oov>' if i == 0 else 'w%d' % i)
    return d


@pytest.mark.parametrize('kind,tied', [('LSTM', False), ('GRU', False), ('GRU', True)])
def test_checkpoint_round_trip(tmp_path, kind, tied):
    import mtl_amd
    lm = mtl_amd.lm
    torch.manual_seed(5)
    V = 37
    model = lm.RNNModel(kind, V, 12, 12 if tied else 20, 2, 0.3, tie_weights=tied)
    with torch.no_grad():
        for p in model.parameters():                                       # (not the flat buffer: its alignment padding stays zero)
            p.add_(torch.randn(p.shape) * 0.01)
    path = str(tmp_path / 'lm.th')
    lm.save_lm_checkpoint(model, _dictionary(V), path)
    back, d = lm.load_lm_checkpoint(path, cuda=False)
    assert (back.rnn_type, back.tie_weights, back.ntoken, back.ninp, back.nhid, back.nlayers) == \
        (kind, tied, V, 12, 12 if tied else 20, 2) and back.drop.p == 0.3 and back.dropout_rate == 0.3
    sa, sb = model.state_dict(), back.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(model.flat_parameters, back.flat_parameters)
    assert (back.decoder.weight is back.encoder.weight) == tied
    assert len(d) == V and d.word2idx['w3'] == 3 and d.idx2word[0] == '<oov>'


def test_checkpoint_loader_refuses_a_wrong_dictionary_and_defaults_to_lstm(tmp_path):
    import mtl_amd
    lm = mtl_amd.lm
    model = lm.RNNModel('LSTM', 21, 8, 8, 1, 0.0)
    path = str(tmp_path / 'lm.th')
    lm.save_lm_checkpoint(model, _dictionary(22), path)                    # one word more than the model's rows
    with pytest.raises(ValueError):
        lm.load_lm_checkpoint(path, cuda=False)
    lm.save_lm_checkpoint(model, _dictionary(21), path)
    ck = torch.load(path)
    del ck['rnn_type']                                                      # the reference's files (lm/convert.py) carry no rnn_type
    torch.save(ck, path)
    back, _ = lm.load_lm_checkpoint(path, cuda=False)
    assert back.rnn_type == 'LSTM' and torch.equal(back.flat_parameters, model.flat_parameters)
    # LMTrainer.train: a corpus that added words to the dictionary is refused before any training (no engine is touched)
    with pytest.raises(ValueError):
        lm.LMTrainer(back, lr=1.0).train(torch.zeros(8, 2, dtype=torch.int64), torch.zeros(8, 2, dtype=torch.int64), 1,
                                         dictionary=_dictionary(22))


def _rank_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import mtl_amd
    mtl_amd.dist.init_from_env(backend='gloo')
    model = mtl_amd.lm.RNNModel('GRU', 11, 4, 4, 1, 0.0)
    got = []
    for make in (lambda: mtl_amd.lm.LMTrainer(model), lambda: mtl_amd.lm.LMJointTrainer(model)):
        try:
            make()
            got.append('built')
        except NotImplementedError:
            got.append('refused')
    ret[rank] = got
    mtl_amd.dist.barrier()


def test_both_trainers_refuse_several_ranks():
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rank_worker, args=(2, 29653, ret), nprocs=2, join=True)
    assert dict(ret) == {0: ['refused', 'refused'], 1: ['refused', 'refused']}
