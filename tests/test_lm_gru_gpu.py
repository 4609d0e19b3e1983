"""GRU and tied-weight language models on the device (csrc/mtl_gru.hip, lm.py) against the fp64 restatement tests/gru_ref.py at
identical parameters, carried state and replayed Philox keep-masks.

Bounds are the ones tests/test_lm.py holds the LSTM to (logits 1e-5 relative norm, loss 1e-6 relative, hidden state 2e-6 absolute,
every gradient tensor 1e-4 by `_errs`, persistent against per-step 2e-6, meta-loop parameters 2e-5); none is wider.  The device's
measured error per shape is recorded in profiles/lm_gru/errors.txt."""
import argparse

import pytest
import torch
import torch.nn.functional as F

from tests import gru_ref as GR

pytestmark = pytest.mark.gpu


def _to_ref(ref, model, flat):
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(model._layout.view(flat, n).cpu())


def _errs(model, flat_g, ref, grads):
    """tests/test_lm.py's measure: per tensor |got - want| / max(|want|, 1e-4 |all gradients|)"""
    gn = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    return {n: float((model._layout.view(flat_g, n).cpu().double() - t).norm() / max(float(t.norm()), 1e-4 * gn))
            for (n, _), t in zip(ref.named_parameters(), grads)}


def _masks(eng, dropout, T, B, E, H, NL):
    if dropout <= 0:
        return None
    sc = 1.0 / (1 - dropout)
    pool = {k[0]: v for k, v in eng.pool.items()}
    masks = {'emb': pool['m_emb'].cpu().double().view(T, B, E) * sc}
    for l in range(NL):
        masks['l%d' % l if l < NL - 1 else 'out'] = pool['m_l%d' % l].cpu().double().view(T, B, H) * sc
    return masks


def _batch(V, T, B, NL, H, seed, lstm=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, V, (T, B), generator=g)
    if T > 1:
        x[T // 2] = x[0]                                                   # repeated ids: the deterministic scatter-add chains
    else:
        x[0, B // 2:] = x[0, 0]
    y = torch.randint(0, V, (T * B,), generator=g)
    h0 = 0.2 * torch.randn(NL, B, H, generator=g)
    return x, y, ((h0, 0.2 * torch.randn(NL, B, H, generator=g)) if lstm else h0)


def _cuda(hidden):
    return hidden.cuda() if torch.is_tensor(hidden) else tuple(h.cuda() for h in hidden)


def _double(hidden):
    return hidden.double() if torch.is_tensor(hidden) else tuple(h.double() for h in hidden)


def _first(hidden):
    return hidden if torch.is_tensor(hidden) else hidden[0]


def _run(model, x, y, hidden, dropout, scale=(1.0,)):
    """forward + backward (once per entry of `scale`, accumulating) -> (logits, loss, new hidden, flat gradient)"""
    eng = model.engine
    torch.manual_seed(77)                                                   # same Philox seed draw -> same keep-masks
    out = eng.forward(model.flat_parameters, x.cuda(), y.cuda(), _cuda(hidden), dropout)
    grad = torch.zeros_like(model.flat_grad)
    for s in scale:
        eng.backward(grad, s)
    torch.cuda.synchronize()
    assert int(eng.sync_ws[1]) == 0, 'a grid-wide wait timed out'
    hid = out['hidden']
    return out['logits'].clone(), float(out['loss']), (hid.clone() if torch.is_tensor(hid) else tuple(h.clone() for h in hid)), grad


def _same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, tuple):
        return all(_same(p, q) for p, q in zip(a, b))
    return a == b


def _reference(ref, x, y, hidden, masks, V):
    out, hn = ref(x, _double(hidden), masks)
    loss = F.cross_entropy(out.view(-1, V), y)
    grads = torch.autograd.grad(loss, list(ref.parameters()))
    return out.detach().view(-1, V), float(loss.detach()), GR.detach(hn), grads


def _check_against_reference(tag, model, ref, res, want):
    logits, loss, hid, grad = res
    o_out, o_loss, o_hid, o_grads = want
    e_log = float((logits.cpu().double() - o_out).norm() / o_out.norm())
    e_loss = abs(loss - o_loss) / o_loss
    e_hid = max(float((a.cpu().double() - b).abs().max()) for a, b in zip((hid,) if torch.is_tensor(hid) else hid,
                                                                          (o_hid,) if torch.is_tensor(o_hid) else o_hid))
    errs = _errs(model, grad, ref, o_grads)
    worst = max(errs.items(), key=lambda kv: kv[1])
    print('lm_gru error %s: logits %.3e loss %.3e hidden %.3e gradient %.3e (%s)' % (tag, e_log, e_loss, e_hid, worst[1], worst[0]))
    assert e_log < 1e-5 and e_loss < 1e-6 and e_hid < 2e-6, tag
    assert worst[1] < 1e-4, (tag, worst)


# ------------------------------------------------------------------------------------------------------------------ cell kernels
@pytest.mark.parametrize('B,H', [(1, 8), (3, 200), (5, 128), (32, 512)])
@pytest.mark.parametrize('masked', [False, True])
def test_gru_cell_kernels(B, H, masked):
    """mtl_gru_cell_fwd / mtl_gru_cell_bwd alone against the restatement in fp64, with and without the dropout mask, the backward
    also in its last-step form (no recurrent gradient, no carry).  Every output is a sum / product of at most eight fp32
    operations (each within an ulp, 6e-8 relative; expf / tanhf a few ulp) on the given inputs: the bound is 1e-6 -- more than ten
    ulp -- times the largest magnitude a result can have: max(1, |h_prev|, |gh|) forward, that times max(1, |dh|) backward (a gate
    gradient is dh times factors bounded by those).  Measured: at most 6e-7, profiles/lm_gru/errors.txt."""
    import mtl_amd
    lib, check = mtl_amd._lib.lib(), mtl_amd._lib.check
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(100 * B + H)
    gx, gh, hp = torch.randn(B, 3 * H, generator=g), torch.randn(B, 3 * H, generator=g), torch.randn(B, H, generator=g)
    keep = (torch.rand(B, H, generator=g) > 0.3).to(torch.uint8)
    msc = 1.0 / 0.7 if masked else 1.0
    d = lambda t: t.cuda().contiguous()
    gx_d, gh_d, hp_d, keep_d = d(gx), d(gh), d(hp), d(keep)
    mp = keep_d.data_ptr() if masked else None
    acts, h, hd = torch.empty(B, 4 * H, device='cuda'), torch.empty(B, H, device='cuda'), torch.empty(B, H, device='cuda')
    check(lib.mtl_gru_cell_fwd(st, gx_d.data_ptr(), gh_d.data_ptr(), hp_d.data_ptr(), acts.data_ptr(), h.data_ptr(), hd.data_ptr(), mp, msc, B, H),
          'gru_cell_fwd')
    w_h, w_acts = GR.gru_cell(gx.double(), gh.double(), hp.double())
    w_hd = w_h * keep.double() * msc if masked else w_h
    tol = 1e-6 * max(1.0, float(hp.abs().max()), float(gh.abs().max()))
    e_f = max(float((acts.cpu().double() - w_acts).abs().max()), float((h.cpu().double() - w_h).abs().max()),
              float((hd.cpu().double() - w_hd).abs().max()))
    print('lm_gru cell error B=%d H=%d masked=%d: forward %.3e (bound %.3e)' % (B, H, masked, e_f, tol))
    assert e_f < tol
    # h_drop is optional
    h2 = torch.empty_like(h)
    check(lib.mtl_gru_cell_fwd(st, gx_d.data_ptr(), gh_d.data_ptr(), hp_d.data_ptr(), acts.data_ptr(), h2.data_ptr(), None, mp, msc, B, H), 'gru_cell_fwd')
    assert torch.equal(h, h2)
    # backward from the device's own saved activations (identical inputs on both sides)
    acts_h = acts.cpu()
    up, rec, car = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    up_d, rec_d, car_d = d(up), d(rec), d(car)
    for last in (False, True):
        dgx, dgh, cout = torch.empty(B, 3 * H, device='cuda'), torch.empty(B, 3 * H, device='cuda'), torch.empty(B, H, device='cuda')
        check(lib.mtl_gru_cell_bwd(st, up_d.data_ptr(), mp, msc, None if last else rec_d.data_ptr(), None if last else car_d.data_ptr(),
                                   acts.data_ptr(), hp_d.data_ptr(), dgx.data_ptr(), dgh.data_ptr(), cout.data_ptr(), B, H), 'gru_cell_bwd')
        dh = up.double() * (keep.double() * msc if masked else 1.0)
        if not last:
            dh = dh + rec.double() + car.double()
        w_dgx, w_dgh, w_c = GR.gru_cell_backward(dh, acts_h.double(), hp.double())
        tol_b = 1e-6 * max(1.0, float(dh.abs().max())) * max(1.0, float(hp.abs().max()), float(gh.abs().max()))
        e_b = max(float((dgx.cpu().double() - w_dgx).abs().max()), float((dgh.cpu().double() - w_dgh).abs().max()),
                  float((cout.cpu().double() - w_c).abs().max()))
        print('lm_gru cell error B=%d H=%d masked=%d last=%d: backward %.3e (bound %.3e)' % (B, H, masked, last, e_b, tol_b))
        assert e_b < tol_b
    # bad arguments are refused before any launch
    assert lib.mtl_gru_cell_fwd(st, None, gh_d.data_ptr(), hp_d.data_ptr(), acts.data_ptr(), h.data_ptr(), None, None, 1.0, B, H) == -22
    assert lib.mtl_gru_cell_bwd(st, up_d.data_ptr(), None, 1.0, None, None, acts.data_ptr(), hp_d.data_ptr(), dgx.data_ptr(), None, cout.data_ptr(), B, H) == -22
    assert lib.mtl_gru_cell_fwd(st, gx_d.data_ptr(), gh_d.data_ptr(), hp_d.data_ptr(), acts.data_ptr(), h.data_ptr(), None, None, 1.0, 0, H) == -22
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- full pass
@pytest.mark.parametrize('H,B,T,dropout,NL,E', [(128, 5, 9, 0.0, 2, 48), (256, 7, 6, 0.3, 3, 48), (384, 32, 4, 0.0, 2, 48), (512, 20, 1, 0.0, 2, 48),
                                                (256, 1, 5, 0.5, 1, 48), (128, 6, 7, 0.3, 2, 128), (256, 4, 5, 0.0, 3, 256),
                                                (512, 20, 35, 0.2, 2, 512), (200, 3, 5, 0.0, 2, 200)])
def test_gru_full_pass(H, B, T, dropout, NL, E):
    """logits, loss, new hidden state and every gradient tensor of one forward + backward: the persistent launches (run twice:
    bitwise equal) and the per-step path, each against the restatement and against each other; T = 1 has no recurrent term, E == H
    has layer 0's input as wide as the state (two weight-gradient products per layer either way), H = 200 (the reference's default
    width) is outside the persistent shapes and must take the per-step path."""
    import mtl_amd
    V = 5120 if E == 512 else 300
    torch.manual_seed(3)
    model = mtl_amd.lm.RNNModel('GRU', V, E, H, NL, dropout).cuda()
    model.train()
    ref = GR.RNNModel('GRU', V, E, H, NL, dropout).double()
    _to_ref(ref, model, model.flat_parameters)
    x, y, h0 = _batch(V, T, B, NL, H, 21 + H)
    eng = model.engine
    supported = bool(eng.lib.mtl_gru_layer_supported(B, H))
    assert supported == (H != 200) and eng.persistent
    runs = {}
    for mode in ('persistent', 'persistent', 'steps'):
        eng.persistent = mode == 'persistent'
        res = _run(model, x, y, h0, dropout)
        assert eng.saved['fused'] == (mode == 'persistent' and supported)
        assert torch.is_tensor(res[2]) and tuple(res[2].shape) == (NL, B, H)
        if mode in runs:
            assert all(_same(a, b) for a, b in zip(res, runs[mode])), 'the persistent launches are not reproducible bit for bit'
        runs[mode] = res
    eng.persistent = True
    want = _reference(ref, x, y, h0, _masks(eng, dropout, T, B, E, H, NL), V)
    tag = 'H=%d B=%d T=%d p=%.1f NL=%d E=%d' % (H, B, T, dropout, NL, E)
    for mode in ('persistent', 'steps'):
        _check_against_reference('%s %s' % (tag, mode), model, ref, runs[mode], want)
    lp, ls = runs['persistent'], runs['steps']
    e_ps = float((lp[3] - ls[3]).norm() / ls[3].norm())
    print('lm_gru error %s persistent-vs-steps: gradient %.3e loss %.3e' % (tag, e_ps, abs(lp[1] - ls[1]) / ls[1]))
    assert e_ps < 2e-6 and abs(lp[1] - ls[1]) < 1e-6 * ls[1]               # the device paths: same arithmetic, other summation orders
    half = _run(model, x, y, h0, dropout, scale=(0.5, 0.5))                 # linear in the loss scale, accumulating
    assert float((half[3] - lp[3]).norm() / lp[3].norm()) < 1e-6
    eng.check_handoff()


# --------------------------------------------------------------------------------------------------------------------------- tied
@pytest.mark.parametrize('rnn_type', ['GRU', 'LSTM'])
def test_tied_full_pass(rnn_type):
    """tie_weights=True: the projection's weight gradient and the embedding scatter-add accumulate into ONE tensor, which must
    equal the restatement's summed gradient of the shared Parameter; every launch mode of either rnn type"""
    import mtl_amd
    H, B, T, dropout, NL, E, V = 128, 5, 9, 0.3, 2, 128, 300
    torch.manual_seed(3)
    model = mtl_amd.lm.RNNModel(rnn_type, V, E, H, NL, dropout, tie_weights=True).cuda()
    model.train()
    assert model.decoder.weight is model.encoder.weight and 'decoder.weight' not in model._layout.entries
    ref = GR.RNNModel(rnn_type, V, E, H, NL, dropout, tie_weights=True).double()
    _to_ref(ref, model, model.flat_parameters)
    assert [n for n, _ in ref.named_parameters()] == model._layout.order
    lstm = rnn_type == 'LSTM'
    x, y, h0 = _batch(V, T, B, NL, H, 5, lstm=lstm)
    eng = model.engine
    modes = {'stack': (True, True), 'layers': (True, False), 'steps': (False, False)} if lstm else {'persistent': (True, True), 'steps': (False, True)}
    runs = {}
    for mode, (persistent, stacked) in modes.items():
        eng.persistent, eng.stacked = persistent, stacked
        runs[mode] = _run(model, x, y, h0, dropout)
        if lstm:
            assert eng.saved['stacked'] == (mode == 'stack')
        else:
            assert eng.saved['fused'] == (mode == 'persistent')
    eng.persistent = eng.stacked = True
    want = _reference(ref, x, y, h0, _masks(eng, dropout, T, B, E, H, NL), V)
    for mode, res in runs.items():
        _check_against_reference('tied %s %s' % (rnn_type, mode), model, ref, res, want)
        got = model._layout.view(res[3], 'encoder.weight').cpu().double()
        assert float((got - want[3][0]).norm() / want[3][0].norm()) < 1e-4    # (parameters()[0] is the shared tensor)
        e = float((res[3] - runs['steps'][3]).norm() / runs['steps'][3].norm())
        assert e < 2e-6 and abs(res[1] - runs['steps'][1]) < 1e-6 * runs['steps'][1], (mode, e)
    eng.check_handoff()


# ------------------------------------------------------------------------------------------------------------------- sequence_nll
@pytest.mark.parametrize('tied', [False, True])
def test_gru_sequence_nll(tied):
    """LMEngine.sequence_nll of a GRU model on a ragged batch (lengths 1, 4, 9; -1 padding targets) against the restatement's
    per-sequence summed NLL: 1e-5 relative, the bound tests/test_lm_rescore_gpu.py holds the LSTM to"""
    import mtl_amd
    V, H, NL, T, B = 300, 128, 2, 9, 3
    torch.manual_seed(13)
    model = mtl_amd.lm.RNNModel('GRU', V, H if tied else 48, H, NL, 0.3, tie_weights=tied).cuda()
    model.eval()
    ref = GR.RNNModel('GRU', V, H if tied else 48, H, NL, 0.3, tie_weights=tied).double()
    _to_ref(ref, model, model.flat_parameters)
    g = torch.Generator().manual_seed(2)
    ids, tgt = torch.randint(0, V, (T, B), generator=g), torch.randint(0, V, (T, B), generator=g)
    for b, n in enumerate((1, 4, 9)):
        tgt[n:, b] = -1
    with torch.no_grad():
        want = ref.sequence_nll(ids, tgt)
    eng = model.engine
    got = {}
    for persistent in (True, False):
        eng.persistent = persistent
        got[persistent] = eng.sequence_nll(model.flat_parameters, ids.cuda(), tgt.cuda()).cpu()
        torch.cuda.synchronize()
        assert int(eng.sync_ws[1]) == 0
    eng.persistent = True
    print('lm_gru error sequence_nll tied=%d: %.3e' % (tied, float(((got[True].double() - want) / want).abs().max())))
    assert torch.allclose(got[True].double(), want, rtol=1e-5, atol=0) and torch.allclose(got[False].double(), want, rtol=1e-5, atol=0)
    with pytest.raises(RuntimeError, match='backward'):
        eng.backward(torch.zeros_like(model.flat_parameters))              # sequence_nll reused forward()'s buffers
    # RNNModel.forward hands a GRU's state back as the single tensor it took
    logits, hid = model(ids.cuda(), model.init_hidden(B))
    assert torch.is_tensor(hid) and tuple(hid.shape) == (NL, B, H) and tuple(logits.shape) == (T, B, V)


# ---------------------------------------------------------------------------------------------------------------------- meta loop
def test_gru_meta_step_matches_restatement():
    """two LMMetaTrainer.run_iteration steps of a GRU model (3 tasks, the single-tensor hidden state carried, clipped inner and outer
    steps, weights 0.1 / 0.1 / 0.8) against gru_ref.meta_step: losses, the second meta-gradient, the parameters after both"""
    import mtl_amd
    from oracle import lm_refimpl as LR                                    # (corpus and dataset helpers only)
    V, E, H = 200, 32, 128
    torch.manual_seed(11)
    model = mtl_amd.lm.RNNModel('GRU', V, E, H, 2, 0.0).cuda()
    model.train()
    ref = GR.RNNModel('GRU', V, E, H, 2, 0.0).double()
    _to_ref(ref, model, model.flat_parameters)
    args = argparse.Namespace(bptt=6, batch_size=4, cuda=False)
    ds = mtl_amd.lm.LMDataset([LR.synth_corpus(s, V, 331) for s in (1, 2, 3)], args)
    tr = mtl_amd.lm.LMMetaTrainer(model, lr=2.0, meta_lr_factor=3.0, clip=0.25, ratio=0.8)
    hid = ref.init_hidden(4)
    for it in (0, 1):
        vb = ds.sample(-1, it)[2:]
        batches = [ds.sample(i, it)[:2] for i in range(3)]
        loss, trl = tr.run_iteration([(x.cuda(), y.cuda()) for x, y in batches], (vb[0].cuda(), vb[1].cuda()))
        G_r, hid, trl_r, val_r = GR.meta_step(ref, hid, batches, vb, 2.0, 3.0, 0.25, 0.8)
        for a, b in zip(trl, trl_r):
            assert abs(a - b) < 1e-5 * b
        assert abs(loss - sum(w * v for w, v in zip(GR.task_weights(3, 0.8), val_r))) < 1e-5 * loss
        errs = _errs(model, tr.G, ref, G_r)
        assert max(errs.values()) < 1e-4, (it, max(errs.items(), key=lambda kv: kv[1]))
        e_p = 0.0
        for n, p in ref.named_parameters():
            q = model._layout.view(model.flat_parameters, n).cpu().double()
            e_p = max(e_p, float((q - p).abs().max()) / max(float(p.abs().max()), 1e-3))
        print('lm_gru error meta loop it=%d: gradient %.3e parameters %.3e' % (it, max(errs.values()), e_p))
        assert e_p < 2e-5, it
        assert torch.is_tensor(tr.hidden) and float((tr.hidden.cpu().double() - hid).abs().max()) < 1e-5
    assert int(model.engine.sync_ws[1]) == 0
