"""Time of the loss stage with --loss ctc at B = 8 utterances, Td = 50 decoder positions, V = 3764:

  * ce_stage   : mtl_ce_argmax_fwd + mtl_ce_bwd -- the loss stage of a ce pass (row log-sum-exp, arg-max, loss; d(logits));
  * ctc_stage  : the loss stage of a ctc pass: the same mtl_ce_argmax_fwd (the pass still needs its arg-max `hyp`), then mtl_ctc_fwd
                 + mtl_ctc_bwd;  ctc_only: the two ctc calls alone;
  * torch_ctc  : F.log_softmax + F.ctc_loss + autograd on the same device -- what a user would run otherwise;
  * with --meta: one meta-iteration (TransientTrainer.meta_iteration, 8 tasks x 8 utterances x 1000 frames x 49 labels, the model of
                 bench.py) with the ce and with the ctc objective.

The paths are timed in alternation: `--rounds` rounds, in each round every path runs one span of `--reps` passes between two device
events; reported per path: the median span (microseconds per pass), the fastest and the slowest.

    python tools/bench_ctc.py [--reps 50] [--rounds 9] [--meta] [--out profiles/ctc_stage.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(B=8, Td=50, V=3764)
META_CFG = dict(num_enc_layers=2, num_dec_layers=4, num_heads=8, dim_model=512, dim_key=64, dim_value=64, dim_inner=512,      # bench.py's CFG
                dim_emb=512, src_max_len=5000, tgt_max_len=2500, r=100, vocab_size=3765)


def span(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3        # microseconds per pass


def stage_paths(mtl_amd):
    lib = mtl_amd._lib.lib()
    B, Td, V = SHAPE['B'], SHAPE['Td'], SHAPE['V']
    rows, ldd = B * Td, (V + 3) // 4 * 4
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, generator=g) * 3).cuda()
    tgt_len = torch.randint(25, Td, (B,), generator=g)
    gold = torch.zeros(B, Td, dtype=torch.int64)
    for u in range(B):
        lab = torch.randperm(V - 4, generator=g)[:int(tgt_len[u])] + 4      # distinct labels: every utterance has an alignment
        gold[u, :int(tgt_len[u])] = lab
        gold[u, int(tgt_len[u])] = 2
    gold_d, tl_d, il_d = gold.cuda(), tgt_len.int().cuda(), torch.full((B,), Td, dtype=torch.int32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device='cuda')
    lse, rowloss, loss, nll, dlog = f32(rows), f32(rows), f32(1), f32(B), f32(rows, ldd)
    hyp = torch.empty(rows, dtype=torch.int64, device='cuda')
    inv = torch.tensor([1.0 / int((gold != 0).sum())], device='cuda')
    ws_bytes = lib.mtl_ctc_workspace(B, Td, Td - 1)
    ws = f32(ws_bytes // 4)

    def ok(rc):
        if rc != 0:
            raise RuntimeError('library call failed: %d' % rc)

    def ce_fwd():
        ok(lib.mtl_ce_argmax_fwd(st, logits.data_ptr(), gold_d.data_ptr(), rows, V, V, 0, 0.0, 0, inv.data_ptr(), lse.data_ptr(),
                                 hyp.data_ptr(), rowloss.data_ptr(), loss.data_ptr()))

    def ce_stage():
        ce_fwd()
        ok(lib.mtl_ce_bwd(st, logits.data_ptr(), lse.data_ptr(), gold_d.data_ptr(), rows, V, V, 0, 0.0, 1.0, inv.data_ptr(), dlog.data_ptr(), ldd))

    def ctc_only():
        ok(lib.mtl_ctc_fwd(st, logits.data_ptr(), gold_d.data_ptr(), il_d.data_ptr(), tl_d.data_ptr(), B, Td, V, V, Td, Td - 1, 0, B,
                           ws.data_ptr(), ws_bytes, nll.data_ptr(), loss.data_ptr()))
        ok(lib.mtl_ctc_bwd(st, logits.data_ptr(), gold_d.data_ptr(), il_d.data_ptr(), tl_d.data_ptr(), B, Td, V, V, Td, Td - 1, 0, B,
                           ws.data_ptr(), ws_bytes, nll.data_ptr(), 1.0, None, dlog.data_ptr(), ldd))

    def ctc_stage():
        ce_fwd()
        ctc_only()

    x3 = logits.view(B, Td, V).clone().requires_grad_(True)
    il_t, tl_t = il_d.long(), tl_d.long()

    def torch_ctc():
        x3.grad = None
        lp = torch.nn.functional.log_softmax(x3.transpose(0, 1), 2)
        torch.nn.functional.ctc_loss(lp, gold_d, il_t, tl_t, blank=0, reduction='mean', zero_infinity=True).backward()

    ctc_only()
    torch_ctc()
    torch.cuda.synchronize()
    ours = dlog.view(B, Td, ldd)[:, :, :V]
    agree = float((ours - x3.grad).abs().max() / x3.grad.abs().max())
    return dict(ce_stage=ce_stage, ctc_stage=ctc_stage, ctc_only=ctc_only, torch_ctc=torch_ctc), agree


def meta_paths(mtl_amd):
    k, T, L, n = 8, 1000, 49, 8
    V = META_CFG['vocab_size']
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
                              emb_trg_sharing=False, label_smoothing=0.0, name='bench_ctc', lr=1e-4, meta_lr=1e-4, k_train=k, k_valid=k,
                              clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_bench', cuda=True,
                              **{a: b for a, b in META_CFG.items() if a not in ('vocab_size', 'r')})
    vocab = mtl_amd.synthetic_vocab(V)
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=META_CFG['r']).cuda()
    as5 = lambda b: (b[0].cuda(), b[1], None, b[2], None)
    tasks = [as5(mtl_amd.synth_batch(10 * m, k, T, L, V)) for m in range(n)]
    val = as5(mtl_amd.synth_batch(71, k, T, L, V))
    inner = mtl_amd.FlatSGD(model, args.lr)
    model.zero_copy_grad()
    trainers = {lt: mtl_amd.TransientTrainer() for lt in ('ce', 'ctc')}

    def path(lt):
        tr = trainers[lt]
        tr.loss_type = lt
        return lambda: tr.meta_iteration(model, vocab, tasks, val, n, inner, None, args)
    return {'meta_' + lt: path(lt) for lt in trainers}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--meta', action='store_true')
    ap.add_argument('--meta-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_stage.json'))
    a = ap.parse_args()
    import mtl_amd
    assert torch.cuda.is_available(), 'bench_ctc needs an MI355X'
    paths, agree = stage_paths(mtl_amd)
    reps = {k: a.reps for k in paths}
    if a.meta:
        meta = meta_paths(mtl_amd)
        paths.update(meta)
        reps.update({k: a.meta_reps for k in meta})
    for k, fn in paths.items():                  # warm-up: code objects, buffer pools, command lists (eager, recorded, replayed)
        span(fn, 4)
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(span(fn, reps[k]))
    res = dict(device=torch.cuda.get_device_name(0), shape=SHAPE, reps=a.reps, rounds=a.rounds, unit='microseconds per pass',
               ctc_vs_torch_gradient_rel=agree,
               paths={k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()})
    med = {k: v['median'] for k, v in res['paths'].items()}
    res['ctc_stage_vs_ce_stage'] = round(med['ctc_stage'] / med['ce_stage'], 3)
    res['torch_vs_ctc_only'] = round(med['torch_ctc'] / med['ctc_only'], 3)
    if a.meta:
        res['meta_ctc_minus_ce_us'] = round(med['meta_ctc'] - med['meta_ce'], 1)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
