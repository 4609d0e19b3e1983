"""Timings for feat_extractor='none' on the MI355X, HIP events after warm-up, one build, one process:

  (a) mtl_featproj_fwd_tb / mtl_featproj_wgrad_tb (csrc/mtl_featproj.hip) at 8 tasks x 8 utterances x 1000 frames, F in {161, 80},
      N in {512, 100}: time and bytes moved per second (forward: x read once + y written; weight gradient: x + dy read once), the
      forward also as a fraction of --hbm-gbs, the achievable HBM rate.  Beside them the only route the product engines offer for
      the same e0: a transposed copy of the batch padded to a multiple of 4 features (torch) and mtl_gemm_f32_tb on a padded weight
      -- timed with the copy inside the span and with the copy made beforehand;
  (b) one meta-step of a `none` model at the north-star configuration (bench.py's: 8 tasks, 8 x 1000 frames, 100 labels, enc 2 /
      dec 4, d 512) beside the vgg_cnn model's step from the same run.

The candidates of a comparison alternate inside every repeat; per candidate the median of the repeats and their spread are printed,
and one JSON line at the end.

    python tools/bench_featnone.py [--repeats 7] [--steps 5] [--hbm-gbs 6300] [--no-step | --no-kernel]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_factorized import CFG, compare  # noqa: E402


def kernel_cases(L, repeats, hbm_gbs, tasks=8, B=8, T=1000):
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for Fq in (161, 80):
        for N in (512, 100):
            g = torch.Generator().manual_seed(Fq * 1000 + N)
            Fp, rows = (Fq + 3) // 4 * 4, B * T
            x = torch.randn(tasks, B, Fq, T, generator=g).cuda()
            per = N * Fq + N                                                   # w | bias per task, at the stride of a theta' stack
            W = (torch.randn(tasks, per, generator=g) / 10).cuda()
            Wp = torch.zeros(tasks, N * Fp + N, device='cuda')                 # the padded weight of the copy route (prepared outside every span)
            Wp[:, :N * Fp].view(tasks, N, Fp)[:, :, :Fq] = W[:, :N * Fq].view(tasks, N, Fq)
            Wp[:, N * Fp:] = W[:, N * Fq:]
            dy = torch.randn(tasks, rows, N, generator=g).cuda()
            y, y2 = torch.empty(tasks, rows, N, device='cuda'), torch.empty(tasks, rows, N, device='cuda')
            dw, dwp = torch.zeros(tasks, per, device='cuda'), torch.zeros(tasks, N, Fp, device='cuda')
            xp = torch.zeros(tasks, rows, Fp, device='cuda')
            ws = torch.empty(8 << 20, device='cuda')
            need = L.mtl_featproj_wgrad_workspace(B, Fq, T, N, tasks)
            wws = torch.empty(need // 4 + 16, device='cuda')

            def fwd():
                rc = L.mtl_featproj_fwd_tb(st, x.data_ptr(), W.data_ptr(), W.data_ptr() + 4 * N * Fq, y.data_ptr(), B, Fq, T, N, tasks, B * Fq * T, per,
                                           rows * N)
                assert rc == 0, rc

            def wgrad():
                rc = L.mtl_featproj_wgrad_tb(st, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), wws.data_ptr(), need, B, Fq, T, N, tasks, B * Fq * T,
                                             rows * N, per)
                assert rc == 0, rc

            def copy():
                xp.view(tasks, B, T, Fp)[..., :Fq].copy_(x.transpose(2, 3))

            def gemm(ta, tb, M, Nn, K, A, lda, Bm, ldb, C, ldc, bias, flags, sA, sB, sC, sbias):
                rc = L.mtl_gemm_f32_tb(st, ta, tb, M, Nn, K, 1.0, A, lda, Bm, ldb, C, ldc, bias, None, 0, flags, tasks, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0,
                                       None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0, tasks, sA, sB, sC, sbias, 0)
                assert rc == 0, rc

            def fwd_gemm():
                gemm(0, 1, rows, N, Fp, xp.data_ptr(), Fp, Wp.data_ptr(), Fp, y2.data_ptr(), N, Wp.data_ptr() + 4 * N * Fp, 0, rows * Fp, N * Fp + N,
                     rows * N, N * Fp + N)

            def wgrad_gemm():
                gemm(1, 0, N, Fp, rows, dy.data_ptr(), N, xp.data_ptr(), Fp, dwp.data_ptr(), Fp, None, 2, rows * N, rows * Fp, N * Fp, 0)
            copy()
            res = compare({'fwd': fwd, 'fwd: copy + gemm': lambda: (copy(), fwd_gemm()), 'fwd: gemm, copy outside': fwd_gemm, 'wgrad': wgrad,
                           'wgrad: copy + gemm': lambda: (copy(), wgrad_gemm()), 'wgrad: gemm, copy outside': wgrad_gemm}, repeats, 20)
            torch.cuda.synchronize()
            err = float((y - y2).norm() / y2.norm())
            assert err < 1e-5, err
            moved = {'fwd': 4.0 * tasks * (B * Fq * T + rows * N), 'wgrad': 4.0 * tasks * (B * Fq * T + rows * N)}
            case = {}
            for k, (med, lo, hi) in res.items():
                gbs = moved[k.split(':')[0]] / med * 1e-3
                frac = ', %.2f of %d GB/s' % (gbs / hbm_gbs, hbm_gbs) if k == 'fwd' else ''
                print('%d x %d x %d frames, F %3d, N %3d  %-26s %8.1f us (%.1f ... %.1f)  %7.1f GB/s of its own operands%s'
                      % (tasks, B, T, Fq, N, k, med, lo, hi, gbs, frac))
                case[k] = dict(us=round(med, 2), min=round(lo, 2), max=round(hi, 2), gbs=round(gbs, 1))
            out['F%d_N%d' % (Fq, N)] = case
    return out


def step_cases(mtl_amd, repeats, steps, n_tasks=8, k=8, T=1000, labels=100):
    dev = torch.device('cuda')
    vocab = mtl_amd.synthetic_vocab(CFG['vocab_size'])

    def build(feat_extractor):
        args = argparse.Namespace(feat_extractor=feat_extractor, sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
                                  emb_trg_sharing=False, label_smoothing=0.0, name='bench_none', lr=1e-4, meta_lr=1e-4, k_train=k, k_valid=k,
                                  clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_bench_none', cuda=True, is_factorized=False,
                                  r=CFG['r'], **{a: b for a, b in CFG.items() if a not in ('vocab_size', 'r')})
        torch.manual_seed(123456)
        model = mtl_amd.init_transformer_model(args, vocab, r=CFG['r']).cuda()
        model.zero_copy_grad()
        return model, args, mtl_amd.TransientTrainer(), mtl_amd.FlatSGD(model, args.lr), mtl_amd.FlatAdam(model, args.meta_lr)

    def batch(seed):
        x, lens, y = mtl_amd.synth_batch(seed, k, T, labels, CFG['vocab_size'])
        return (x.to(dev), lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32))
    local, val = [batch(10 * m) for m in range(n_tasks)], batch(10 * (n_tasks - 1) + 1)
    none, vgg = build('none'), build('vgg_cnn')

    def step(which):
        model, args, trainer, inner, outer = which
        trainer.run_iteration(model, vocab, local, val, n_tasks, inner, outer, args)
    res = compare({'none (1000 positions)': lambda: step(none), 'vgg_cnn (250 positions)': lambda: step(vgg)}, repeats, steps, warmup=4)
    for name, (med, lo, hi) in res.items():
        print('meta-step, %d tasks  %-26s %9.2f ms (%.2f ... %.2f)' % (n_tasks, name, med / 1e3, lo / 1e3, hi / 1e3))
    return {name: dict(ms=round(med / 1e3, 3), min=round(lo / 1e3, 3), max=round(hi / 1e3, 3)) for name, (med, lo, hi) in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5, help='meta-steps per timed window')
    ap.add_argument('--hbm-gbs', type=float, default=6300.0, help='the HBM rate taken as achievable (GB/s): the forward is reported as a fraction of it')
    ap.add_argument('--no-step', action='store_true', help='kernel comparison only')
    ap.add_argument('--no-kernel', action='store_true', help='meta-step comparison only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_featnone.py measures on an MI355X: no device found')
    import mtl_amd
    out = {} if a.no_kernel else dict(kernel=kernel_cases(mtl_amd._lib.lib(), a.repeats, a.hbm_gbs))
    if not a.no_step:
        out['meta_step'] = step_cases(mtl_amd, a.repeats, a.steps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
