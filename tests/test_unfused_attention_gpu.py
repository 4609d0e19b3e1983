"""MI355X: the attention path of models the fused kernel does not serve -- every (dim_key, dim_value) other than (64, 64) and (16, 16).
Kernel level: mtl_softmax_mask_fwd / mtl_softmax_bwd against torch float64, row by row, at the row lengths where the kernel's 64-key
stride takes a second step and at the leading dimensions the decode session uses.
Engine level: two small models against the live CPU oracle -- A (d_k = d_v = 32: grouped projections, cross K/V plan) and
B (d_k = 16, d_v = 32: h d_k != h d_v, projections one by one, no plan, two gather tables) -- through one pass, a pass with dropout,
a meta-iteration on per-task lanes, the greedy search and both beam searches.  Bars: the ones the project already uses for each of these
(tests/test_ops_gpu.py::test_softmax, tests/test_parity_gpu.py, tests/test_beam_device_gpu.py); none is set from a measurement here.
A model with d_k > d_v is NOT covered: there a missed V-side stride would read beyond a buffer instead of failing a comparison."""
import numpy as np
import pytest
import torch

from tests import beam_util as bu
from tests import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the softmax kernels
FWD_BAR, BWD_BAR = 2e-6, 1e-5      # per ROW here (test_softmax: the same two numbers on the whole tensor)
SCALE, P_DROP = 0.25, 0.3
SHAPES = [(1, 1, 0),               # one key
          (1, 73, 0),              # the decode call
          (5, 63, 0),              # one key below a wave
          (9, 64, 0),              # exactly one wave
          (3, 65, 0),              # one key above a wave
          (70, 70, 1),             # causal
          (130, 130, 1),           # causal
          (2, 257, 0),             # five strides
          (1, 300, 0)]             # the decode call, long row
_REF = {}


def _reference(Tq, Tk, causal, with_klen, ld):
    """inputs and the float64 reference of one case, computed once and left unchanged: scores, upstream gradient, blocked keys, P,
    and per dropout setting (keep mask or None) the probabilities that feed P.V and dS"""
    key = (Tq, Tk, causal, with_klen, ld)
    if key in _REF:
        return _REF[key]
    Bn, H = 3, 2
    g = torch.Generator().manual_seed(1000 * Tq + 10 * Tk + causal)
    s = torch.randn(Bn, H, Tq, Tk, generator=g) * 3
    dp = torch.randn(Bn, H, Tq, Tk, generator=g)
    klen = torch.tensor([Tk, max(1, Tk // 2), 1], dtype=torch.int32) if with_klen else None
    blocked = torch.zeros(Bn, 1, Tq, Tk, dtype=torch.bool)
    if klen is not None:
        blocked = blocked | (torch.arange(Tk).view(1, 1, 1, Tk) >= klen.view(Bn, 1, 1, 1))
    if causal:
        blocked = blocked | torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), 1)
    blocked = blocked.expand(Bn, H, Tq, Tk).contiguous()
    seed = torch.tensor([99], dtype=torch.int64).cuda()
    mask = torch.empty(Bn, H, Tq, ld, dtype=torch.uint8).cuda()
    import mtl_amd
    assert mtl_amd._lib.lib().mtl_dropout_mask(st(), mask.data_ptr(), mask.numel(), P_DROP, seed.data_ptr(), 3 << 40) == 0
    keep = mask.cpu()[..., :Tk].double()
    ref = {}
    for drop in (False, True):
        sr = s.double().requires_grad_(True)
        p = torch.softmax((sr * SCALE).masked_fill(blocked, -np.inf), -1)
        pd = p * keep * (1.0 / (1.0 - P_DROP)) if drop else p
        pd.backward(dp.double())
        ref[drop] = (p.detach(), pd.detach(), sr.grad.detach())
    _REF[key] = dict(s=s, dp=dp, klen=klen, blocked=blocked, mask=mask, ref=ref)
    return _REF[key]


def _row_errors(got, ref):
    """relative L2 error of every row; a row's denominator: max(its own norm, 1e-3 x the largest row norm of the tensor)"""
    got, ref = got.double().cpu().reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    norms = ref.norm(dim=1)
    return (got - ref).norm(dim=1) / torch.maximum(norms, 1e-3 * norms.max()).clamp_min(1e-300)


def _run_softmax(L, case, Tq, Tk, causal, ld, drop):
    """forward and backward on fresh buffers whose columns [Tk, ld) (and the whole dropped copy) hold NaN -> (P, Pd or None, dS)"""
    Bn, H = 3, 2
    nan = float('nan')
    S = torch.full((Bn, H, Tq, ld), nan)
    S[..., :Tk] = case['s']
    D = torch.full((Bn, H, Tq, ld), nan)
    D[..., :Tk] = case['dp']
    S, D = S.cuda(), D.cuda()
    Pd = torch.full((Bn, H, Tq, ld), nan).cuda() if drop else None
    kd = case['klen'].cuda() if case['klen'] is not None else None
    m = case['mask'].data_ptr() if drop else None
    pscale = 1.0 / (1.0 - P_DROP) if drop else 1.0
    assert L.mtl_softmax_mask_fwd(st(), S.data_ptr(), kd.data_ptr() if kd is not None else None, causal, SCALE, Bn, H, Tq, Tk, ld, m, pscale,
                                  Pd.data_ptr() if drop else None) == 0
    assert L.mtl_softmax_bwd(st(), S.data_ptr(), D.data_ptr(), SCALE, Bn * H * Tq, Tk, ld, m, pscale) == 0
    torch.cuda.synchronize()
    return S.cpu(), Pd.cpu() if drop else None, D.cpu()


def _check_softmax(L, Tq, Tk, causal, wide, drop, with_klen=True):
    ld = (Tk + 3) // 4 * 4 + (12 if wide else 0)
    case = _reference(Tq, Tk, causal, with_klen, ld)
    p_ref, pd_ref, ds_ref = case['ref'][drop]
    blocked = case['blocked']
    P, Pd, dS = _run_softmax(L, case, Tq, Tk, causal, ld, drop)
    e_p = float(_row_errors(P[..., :Tk], p_ref).max())
    e_pd = float(_row_errors(Pd[..., :Tk], pd_ref).max()) if drop else 0.0
    e_ds = float(_row_errors(dS[..., :Tk], ds_ref).max())
    print('softmax Tq %d Tk %d causal %d ld %d drop %d klen %d: worst row P %.2e, dropped copy %.2e, dS %.2e'
          % (Tq, Tk, causal, ld, drop, with_klen, e_p, e_pd, e_ds))
    assert e_p < FWD_BAR and e_pd < FWD_BAR and e_ds < BWD_BAR
    # masked keys: exact zeros in P, the dropped copy and dS, not rounding noise
    for t in (P, Pd, dS):
        if t is not None:
            assert float(t[..., :Tk][blocked].abs().sum()) == 0.0
    # rows with a single visible key: P = 1, so dS = P (dP - P dP) is exactly zero
    single = (~blocked).sum(-1) == 1
    if bool(single.any()):
        assert float(dS[..., :Tk][single].abs().max()) == 0.0 and float(ds_ref[single].abs().max()) == 0.0
    else:
        assert not with_klen and not causal and Tk > 1
    # the columns between Tk and ld belong to nobody: the sentinel is still there
    for t in (P, Pd, dS):
        if t is not None and ld > Tk:
            assert bool(torch.isnan(t[..., Tk:]).all())
    assert not bool(torch.isnan(P[..., :Tk]).any()) and not bool(torch.isnan(dS[..., :Tk]).any())
    # bitwise repeatable
    P2, Pd2, dS2 = _run_softmax(L, case, Tq, Tk, causal, ld, drop)
    assert torch.equal(P[..., :Tk], P2[..., :Tk]) and torch.equal(dS[..., :Tk], dS2[..., :Tk])
    if drop:
        assert torch.equal(Pd[..., :Tk], Pd2[..., :Tk])


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('Tq,Tk,causal', SHAPES)
def test_softmax_rows_against_float64(L, Tq, Tk, causal, wide, drop):
    """every row of P, of the dropped copy and of dS against softmax((s scale).masked_fill(blocked, -inf)) and autograd in float64:
    B = 3, H = 2, klen = [Tk, max(1, Tk // 2), 1], scores randn * 3, scale 0.25; ld = Tk rounded to 4 and that + 12 (the decode
    session's ldS is wider than its rows); without and with a dropout mask (p = 0.3).  torch's fp32 softmax on the same inputs
    (CPU) stays below 1.5e-7 per row forward and 2.4e-6 backward (130 x 130 causal).
    Measured on an MI355X over all cases, the worst rows: P 1.52e-7, dropped copy 1.80e-7, dS 6.30e-7 (130 x 130 causal)."""
    _check_softmax(L, Tq, Tk, causal, wide, drop)


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('Tq,Tk,causal', [(3, 65, 0), (70, 70, 1)])
def test_softmax_rows_without_key_lengths(L, Tq, Tk, causal, drop):
    """klen = None, as the decode session calls the kernel: every key up to Tk (up to q when causal) is visible"""
    _check_softmax(L, Tq, Tk, causal, True, drop, with_klen=False)


# ------------------------------------------------------------------------------------------------ two models off the fused path
SHARED = dict(num_enc_layers=2, num_dec_layers=2, num_heads=4, dim_model=64, dim_inner=128, dim_emb=64, src_max_len=500, tgt_max_len=100,
              vocab_size=64, r=20)
CFG = {'A': dict(SHARED, dim_key=32, dim_value=32),      # one 'qkv' / 'kv' group per block, cross K/V plan
       'B': dict(SHARED, dim_key=16, dim_value=32)}      # h d_k != h d_v: projections one by one, no plan, two gather tables
SPEC = dict(k=3, lr=0.01, meta_lr=0.001)
PASS_BATCH = (7, 3, 288, 70, 64, True)      # lengths 288 / 172 / 36: T4 = 72 keys, 70 labels = 71 decoder positions: every kind of softmax row > a wave
MIN_MARGIN = 1e-3                           # tests/test_beam_device_gpu.py


def _model(name, perturb=None):
    from tests.test_parity_gpu import make
    cfg = CFG[name]
    mtl_amd, args, vocab, model = make(cfg, SPEC, name='unfused')
    if perturb is not None:
        gu.perturb_output_layer(model.decoder.output_linear.weight, perturb)
    model = model.cuda()
    _off_the_fused_path(name, model)
    return mtl_amd, args, vocab, model, cfg


def _off_the_fused_path(name, model):
    from mtl_amd import passplan
    eng = model.engine
    assert not eng.fused_attn
    groups = [g[0] for g in passplan.qkv_groups(eng.L, 'decoder.layers.0.self_attn.', 1, 1, 1, 1, eng.hp.h * eng.hp.dk, eng.hp.h * eng.hp.dv)]
    assert groups == (['qkv'] if name == 'A' else ['q', 'k', 'v'])
    assert (passplan.cross_kv_plan(eng.L, eng.hp.n_dec, eng.hp.dk, eng.hp.dv) is not None) == (name == 'A')


def _oracle(name, perturb=None):
    from oracle import refimpl as R
    oracle = R.build_model(CFG[name])
    if perturb is not None:
        gu.perturb_output_layer(oracle.decoder.output_linear.weight, perturb)
    return oracle


@pytest.mark.parametrize('name,labels', [('A', 70), ('B', 70), ('B', 71)])
def test_one_pass_against_live_oracle(name, labels):
    """product + mtl_softmax_mask_fwd + product forward, five products + mtl_softmax_bwd backward, in the encoder (72 keys, lengths
    72 / 43 / 9), the causal decoder self-attention (71) and the cross-attention (71 x 72): labels bit-exact, logits 1e-5, loss and every
    gradient tensor 1e-4 with the device's branch decisions replayed (tests/test_parity_gpu.py::_pass_parity).
    Model B a second time with 71 labels: 72 decoder positions = 72 encoder positions, the one shape at which layer 0's decoder
    self-attention backward (side stream) and the encoder's (main stream) ask for score-gradient buffers of the same size.
    Measured on an MI355X: A 0 branch near-ties decided differently, worst gradient tensor 3.6e-6 (d0 encoder_attn.query_linear_b.weight);
    B 2 near-ties (margin 4.5e-8), worst 6.6e-6 (d1 encoder_attn.key_linear_b.bias); 122 / 122 tensors within 1e-4 in both."""
    from oracle import refimpl as R
    from tests.test_parity_gpu import _pass_parity
    mtl_amd, args, vocab, model, cfg = _model(name)
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in _oracle(name).named_parameters()]
    batch = R.synth_batch(*PASS_BATCH[:3], labels, *PASS_BATCH[4:])
    assert batch[1].tolist() == ([288, 172, 36] if labels == 70 else [288, 248, 36]) and int((batch[2] != 0).sum(1).max()) == labels
    _pass_parity(model, _oracle(name), batch, model.flat_parameters, 'model %s one pass, %d labels' % (name, labels))
    A, Td = model.engine.arena, labels + 1
    assert A['e0.sa.P'].shape == (3, 4, 72, 72) and A['d1.sa.P'].shape == (3, 4, Td, 72) and A['d1.ca.P'].shape == (3, 4, Td, 72)
    assert (A.get('xkv.plan') is not None) == (name == 'A')


def test_dropout_pass_with_the_same_masks():
    """model B with dropout 0.1: the only place the unfused path's `Pd` buffer is used -- the dropped probabilities feed P.V and dV, the
    un-dropped ones the softmax backward.  The body and the bars are those of
    tests/test_parity_gpu.py::test_dropout_pass_matches_oracle_with_the_same_masks.
    Measured on an MI355X: worst gradient tensor 7.6e-6 (d1 encoder_attn.key_linear_b.bias)."""
    from oracle import refimpl as R
    from tests.test_parity_gpu import _dropout_pass_parity
    model, errs = _dropout_pass_parity(CFG['B'], SPEC, R.synth_batch(*PASS_BATCH), on_model=lambda m: _off_the_fused_path('B', m))
    worst = max(errs, key=errs.get)
    print('model B dropout pass: worst gradient tensor %.2e (%s)' % (errs[worst], worst))
    assert not model.engine.fused_attn


@pytest.mark.parametrize('name', ['A', 'B'])
def test_meta_iteration_on_lanes_against_live_oracle(name):
    """two tasks and a validation batch at the shape of the one-pass test: the trainer must take the per-task lanes (the task-batched
    pass needs the fused kernel), model._G must equal the sum of the single passes' gradients -- train pass at theta0, validation pass at
    theta', each checked against the oracle on the way -- within the per-lane bar of
    tests/test_parity_gpu.py::test_every_pass_of_a_meta_step_against_live_oracle (2e-6 when no branch decision differs, 1e-4 otherwise),
    and three further iterations on the same batches (eager with command lists on, recording, replay) give the first one's G bit for bit.
    Measured on an MI355X: A and B |G - sum of passes| / |G| = 0 with no decision different (the lanes run the single passes' kernels);
    the eight single passes: 0 to 4 near-ties against the free-running oracle, worst gradient tensor 1.1e-5 (A) and 7.4e-6 (B)."""
    from oracle import refimpl as R
    from oracle import branches
    from tests.test_parity_gpu import _pass_parity, _decisions_that_differ, LAST_GATES
    mtl_amd, args, vocab, model, cfg = _model(name)
    oracle = _oracle(name)
    n = 2
    tr = [R.synth_batch(PASS_BATCH[0] + 1 + m, *PASS_BATCH[1:]) for m in range(n)]
    val = R.synth_batch(PASS_BATCH[0] + 10, *PASS_BATCH[1:])
    inner = mtl_amd.FlatSGD(model, SPEC['lr'])
    G_sum = torch.zeros_like(model.flat_grad)
    single = []
    for m, batch in enumerate(tr):
        g_tr, _ = _pass_parity(model, oracle, batch, model.flat_parameters, 'model %s task %d train' % (name, m))
        single.append(LAST_GATES[0])
        theta1 = inner.theta_prime_from(model.flat_parameters, g_tr).clone()
        g_val, _ = _pass_parity(model, oracle, val, theta1, 'model %s task %d valid' % (name, m))
        single.append(LAST_GATES[0])
        G_sum += g_tr + g_val / n
    trainer = mtl_amd.TransientTrainer()
    model.zero_copy_grad()
    as5 = lambda b: (b[0].cuda(), b[1], None, b[2], None)
    tasks, vb = [as5(b) for b in tr], as5(val)
    assert all(not e.fused_attn for e in model.engines[:n])
    with branches.capture_gates(model) as log:
        trainer.meta_iteration(model, vocab, tasks, vb, n, inner, None, args)        # (no NotImplementedError from mha_fwd)
        torch.cuda.synchronize()
    assert trainer.last_schedule == 'lanes'
    flips = _decisions_that_differ(single, log, SPEC['k'])
    comp = float((model._G - G_sum).norm() / G_sum.norm())
    print('model %s composition (per-task lanes): |G - sum of passes| / |G| = %.2e, %d decisions differ' % (name, comp, flips))
    assert len(log) == 2 * n
    assert comp < (2e-6 if flips == 0 else 1e-4), (comp, flips)
    G0 = model._G.clone()
    for rnd in range(3):
        trainer.meta_iteration(model, vocab, tasks, vb, n, inner, None, args)
        torch.cuda.synchronize()
        assert trainer.last_schedule == 'lanes' and torch.equal(model._G, G0), rnd
    recorded = trainer.replay.recorded()
    assert len(recorded) == n and all(cl.n > 100 for cl in recorded)             # one list per lane, and it was replayed


# (model, seed) of R.synth_batch(seed, 4, 288, 6, 64, True) and the smallest top-2 gap of the oracle's log-probabilities over the 4 rows
# and 40 steps of its greedy search (tests/beam_util.py oracle_greedy_margin), with B0's perturbation of the vocabulary projection on.
# Seeds 3000 .. 3009 were looked at on the CPU and these kept for margins >= 1e-3 (A: 3004 has 1.1e-4, B: 3008 has 8.4e-4): a property
# of the inputs, asserted below, not a measurement of the device.
GREEDY_CASES = [('A', 3002, 1.2846e-02), ('A', 3006, 3.8855e-02), ('B', 3004, 2.6865e-02), ('B', 3001, 3.5512e-02)]
GREEDY_STEPS = 40


@pytest.mark.parametrize('name,seed,margin', GREEDY_CASES)
def test_greedy_search_matches_the_cpu_oracle(name, seed, margin):
    """Transformer.evaluate -> greedy_decode on the non-fast decode._DecodeSession: per step three _lowrank products into row t of the K / V
    caches ((B, S, h d_k) and (B, S, h d_v): two row widths in model B) and _attend over t + 1 cached rows and over the 72 rows of each
    utterance's own memory -- four utterances, 40 steps, ids equal to oracle.refimpl.greedy_search; eager, recorded and replayed."""
    from oracle import refimpl as R
    bspec = gu.load_beam()[0]
    mtl_amd, args, vocab, model, cfg = _model(name, bspec)
    oracle = _oracle(name, bspec)
    x, lens, y = R.synth_batch(seed, 4, 288, 6, cfg['vocab_size'], True)
    got_margin = bu.oracle_greedy_margin(oracle, x, lens, vocab.SOS_ID, GREEDY_STEPS)
    print('model %s seed %d greedy: margin %.4e (recorded %.4e)' % (name, seed, got_margin, margin))
    assert margin >= MIN_MARGIN and got_margin >= MIN_MARGIN and abs(got_margin - margin) <= 0.05 * margin
    ref = R.greedy_search(oracle, x, lens, vocab.SOS_ID, GREEDY_STEPS)             # (B, steps)
    for rnd in range(3):
        model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=GREEDY_STEPS)
        assert torch.equal(model.last_greedy_ids.t().contiguous(), ref), rnd
    keys = model.engine.replay_greedy.keys()
    assert len(keys) == 1 and keys[0][-1] is False                                   # the session was not the `fast` one
    assert len(model.engine.replay_greedy.recorded(keys[0])) == 1                    # ... and its steps were recorded and replayed


# (model, seed) of R.synth_batch(seed, 4, 288, 6, 64, True) and the batch's smallest decision margin on the CPU oracle at W = 3
# (tests/beam_util.py oracle_beam_margin), B0's perturbation on; as ORACLE_CASES of tests/test_beam_device_gpu.py
BEAM_CASES = [('A', 3002, 2.5101e-03), ('A', 3003, 1.5593e-03), ('A', 3004, 3.5982e-03), ('B', 3004, 8.5907e-03)]
BEAM_W, BEAM_NBEST = 3, 2


@pytest.mark.parametrize('name,seed,margin', BEAM_CASES)
def test_beam_searches_match_the_cpu_oracle(name, seed, margin):
    """beam_decode (one utterance per session, the W rows share one memory: _attend with batch stride 0 on both caches) and
    beam_decode_batch (4 utterances per step: _attend_groups, mtl_beam_gather on one table for A and two for B) against
    oracle.refimpl.beam_search: ids equal, scores within 1e-4 max(1, |score|), a repeated search equal to the first.  Most hypotheses
    run to the forced EOS at position 72, so the self-attention rows grow past 64 keys."""
    from oracle import refimpl as R
    from tests.test_beam_device_gpu import _memory
    bspec = gu.load_beam()[0]
    mtl_amd, args, vocab, model, cfg = _model(name, bspec)
    oracle = _oracle(name, bspec)
    k, W, nbest, tgt = 4, BEAM_W, BEAM_NBEST, cfg['tgt_max_len']
    x, lens, y = R.synth_batch(seed, k, 288, 6, cfg['vocab_size'], True)
    got_margin = bu.oracle_beam_margin(oracle, x, lens, vocab.SOS_ID, W, tgt, vocab.EOS_ID)
    print('model %s seed %d W %d: margin %.4e (recorded %.4e)' % (name, seed, W, got_margin, margin))
    assert margin >= MIN_MARGIN and got_margin >= MIN_MARGIN and abs(got_margin - margin) <= 0.05 * margin
    eng, theta = model.engine, model.flat_parameters
    assert eng.beam_chunk(W) > 1                                                     # several utterances per decoder step
    nw = gu.label_words(vocab.id2label, [vocab.PAD_TOKEN, vocab.SOS_TOKEN, vocab.EOS_TOKEN])
    ref = R.beam_search(oracle, x, lens, vocab.SOS_ID, W, nbest, tgt, nw)
    ref_ids = [[seq for seq, _ in utt] for utt in ref]
    assert max(len(seq) for utt in ref_ids for seq in utt) > 66                      # start token + more than 64 cached rows + EOS
    mem, T4 = _memory(model, x, lens, y)
    assert T4 == 72
    assert len(eng.decode_session(theta, mem.data_ptr(), k * W, T4, tgt, shared_memory=True, groups=k).gather_tables()) == (1 if name == 'A' else 2)

    def close(res):
        assert [[seq for seq, _ in utt] for utt in res] == ref_ids
        for utt, rutt in zip(res, ref):
            for (_, sc), (_, rsc) in zip(utt, rutt):
                assert abs(sc - rsc) <= 1e-4 * max(1.0, abs(rsc))
    batch = lambda: eng.beam_decode_batch(theta, mem.data_ptr(), k, T4, vocab.SOS_ID, W, nbest, tgt, model._num_words, vocab.EOS_ID, 1.0)
    host = lambda: [eng.beam_decode(theta, mem.data_ptr() + 4 * b * T4 * eng.hp.d, T4, vocab.SOS_ID, W, nbest, tgt, model._num_words,
                                    vocab.EOS_ID, 1.0) for b in range(k)]
    dev = batch()
    close(dev)
    hst = host()
    close(hst)
    assert batch() == dev and batch() == dev                                         # recorded and replayed command lists
    assert host() == hst
    for replay in (eng.replay_beam_batch, eng.replay_beam):                          # neither session was the `fast` one
        assert replay.keys() and all(key[-1] is False for key in replay.keys())
    assert eng.replay_beam_batch.recorded()
