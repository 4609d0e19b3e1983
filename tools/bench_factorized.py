"""Timings for --is-factorized on the MI355X, HIP events after warm-up, one build, one process:

  * mtl_ffn_lr_mid_fwd (csrc/mtl_ffn_lr.hip) against the two-call route it replaces (mtl_gemm_f32_ex with bias + ReLU, then a second
    call; task-batched: mtl_gemm_f32_tb) at rows = 808, tasks in {1, 8}, r = 100, inner in {512, 2048}, h stored and not stored;
  * one factorized meta-step at the north-star configuration (bench.py's: 8 tasks, 8 x 1000 frames, 100 labels, enc 2 / dec 4, d 512,
    inner 512, r 100) with PassEngine.ffn_mid_fused on and off, and beside them the dense model's step from the same run.

The candidates of a comparison alternate inside every repeat, so a clock that drifts moves all of them; per candidate the median of
the repeats and their spread (min ... max) are printed, and one JSON line at the end.

    python tools/bench_factorized.py [--repeats 7] [--steps 5] [--no-step | --no-kernel]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CFG = dict(num_enc_layers=2, num_dec_layers=4, num_heads=8, dim_model=512, dim_key=64, dim_value=64, dim_inner=512, dim_emb=512,
           src_max_len=5000, tgt_max_len=2500, r=100, vocab_size=3765)


def timed(fn, inner):
    """device time of `inner` back-to-back calls of fn, in microseconds per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def compare(cands, repeats, inner, warmup=3):
    """{name: fn} -> {name: (median, min, max)} with the candidates alternating inside every repeat"""
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cands}
    for _ in range(repeats):
        for k, fn in cands.items():
            samples[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def kernel_cases(L, repeats):
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for tasks in (1, 8):
        for inner in (512, 2048):
            rows, r = 808, 100
            g = torch.Generator().manual_seed(tasks * 10000 + inner)
            a = torch.randn(tasks, rows, r, generator=g).cuda()
            per = inner * r + inner + r * inner
            W = (torch.randn(tasks, per, generator=g) / 10).cuda()            # B1 | b1 | A2 per task, at the stride of a theta' stack
            pB1, pb1, pA2 = W.data_ptr(), W.data_ptr() + 4 * inner * r, W.data_ptr() + 4 * (inner * r + inner)
            h, c = torch.empty(tasks, rows, inner, device='cuda'), torch.empty(tasks, rows, r, device='cuda')
            h2, c2 = torch.empty_like(h), torch.empty_like(c)
            ws = torch.empty(8 << 20, device='cuda')

            def fused(store):
                rc = L.mtl_ffn_lr_mid_fwd(st, a.data_ptr(), r, pB1, pb1, pA2, h.data_ptr() if store else None, c.data_ptr(), r, rows, r, inner, tasks,
                                          rows * r, per, rows * inner, rows * r)
                assert rc == 0, rc

            def gemm(M, N, K, A, B, C, bias, flags, sA, sC):
                head = (st, 0, 1, M, N, K, 1.0, A, K, B, K, C, N, bias, None, 0, flags)
                if tasks == 1:
                    rc = L.mtl_gemm_f32_ex(*head, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0)
                else:       # the engine's task-batched call: one item per task, weights and bias at the task stride
                    rc = L.mtl_gemm_f32_tb(*head, tasks, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0, tasks, sA, per, sC,
                                           per, 0)
                assert rc == 0, rc

            def two_call():
                gemm(rows, inner, r, a.data_ptr(), pB1, h2.data_ptr(), pb1, 1, rows * r, rows * inner)
                gemm(rows, r, inner, h2.data_ptr(), pA2, c2.data_ptr(), None, 0, rows * inner, rows * r)
            res = compare({'fused, h stored': lambda: fused(True), 'fused, h not stored': lambda: fused(False), 'two calls': two_call}, repeats, 50)
            torch.cuda.synchronize()
            err = float((c - c2).norm() / c2.norm())
            assert err < 1e-5, err
            flops = 4.0 * tasks * rows * r * inner
            for k, (med, lo, hi) in res.items():
                print('rows 808 x %d tasks, r 100, inner %4d  %-20s %8.1f us (%.1f ... %.1f)  %6.1f TFLOP/s' % (tasks, inner, k, med, lo, hi, flops / med * 1e-6))
            out['tasks%d_inner%d' % (tasks, inner)] = {k: dict(us=round(med, 2), min=round(lo, 2), max=round(hi, 2)) for k, (med, lo, hi) in res.items()}
    return out


def step_cases(mtl_amd, repeats, steps, n_tasks=8, k=8, T=1000, labels=100):
    dev = torch.device('cuda')
    vocab = mtl_amd.synthetic_vocab(CFG['vocab_size'])

    def build(factorized):
        args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
                                  emb_trg_sharing=False, label_smoothing=0.0, name='bench_fz', lr=1e-4, meta_lr=1e-4, k_train=k, k_valid=k, clip=False,
                                  max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_bench_fz', cuda=True, is_factorized=factorized, r=CFG['r'],
                                  **{a: b for a, b in CFG.items() if a not in ('vocab_size', 'r')})
        torch.manual_seed(123456)
        model = mtl_amd.init_transformer_model(args, vocab, is_factorized=factorized, r=CFG['r']).cuda()
        model.zero_copy_grad()
        return model, args, mtl_amd.TransientTrainer(), mtl_amd.FlatSGD(model, args.lr), mtl_amd.FlatAdam(model, args.meta_lr)

    def batch(seed):
        x, lens, y = mtl_amd.synth_batch(seed, k, T, labels, CFG['vocab_size'])
        return (x.to(dev), lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32))
    local, val = [batch(10 * m) for m in range(n_tasks)], batch(10 * (n_tasks - 1) + 1)
    fz, dense = build(True), build(False)

    def step(which, fused=None):
        model, args, trainer, inner, outer = which
        if fused is not None:
            for e in model.engines:
                e.ffn_mid_fused = fused
        trainer.run_iteration(model, vocab, local, val, n_tasks, inner, outer, args)
    # (a trainer keys its command lists on the engine's routing: switching ffn_mid_fused between steps would replay the other route, so
    # each route gets a trainer of its own on the shared model)
    fz_off = (fz[0], fz[1], mtl_amd.TransientTrainer(), fz[3], fz[4])
    cands = {'factorized, fused': lambda: step(fz, True), 'factorized, two calls': lambda: step(fz_off, False), 'dense': lambda: step(dense)}
    res = compare(cands, repeats, steps, warmup=4)
    for name, (med, lo, hi) in res.items():
        print('meta-step, %d tasks  %-24s %9.2f ms (%.2f ... %.2f)' % (n_tasks, name, med / 1e3, lo / 1e3, hi / 1e3))
    return {name: dict(ms=round(med / 1e3, 3), min=round(lo / 1e3, 3), max=round(hi / 1e3, 3)) for name, (med, lo, hi) in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5, help='meta-steps per timed window')
    ap.add_argument('--no-step', action='store_true', help='kernel comparison only')
    ap.add_argument('--no-kernel', action='store_true', help='meta-step comparison only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_factorized.py measures on an MI355X: no device found')
    import mtl_amd
    out = {} if a.no_kernel else dict(kernel=kernel_cases(mtl_amd._lib.lib(), a.repeats))
    if not a.no_step:
        out['meta_step'] = step_cases(mtl_amd, a.repeats, a.steps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
