"""Timings of LM rescoring on the device (DESIGN.md "Beam search with LM rescoring"):

  * the fused sequence NLL (mtl_lm_nll_fwd) against the two-step path it replaces (logits by mtl_gemm_f32_ex, then
    mtl_ce_argmax_fwd) at the reference LM's size (V = 30011 words, H = 200 and 650, R = T B = 256 rows), with the fraction of the
    exact-fp32 MFMA roof (2 R V H FLOP at 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz);
  * Transformer.evaluate(beam_search=True) on the tests/golden/R0.npz batch without and with rescoring by an LM of that size.

    python tools/bench_lm_rescore.py [--reps 50]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MFMA_ROOF = 256 * 4 * 64 * 2.4e9


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def kernel_bench(L, R, H, V, reps):
    g = torch.Generator().manual_seed(0)
    x = torch.tanh(torch.randn(R, H, generator=g)).cuda()
    W = (0.15 * torch.randn(V, H, generator=g)).cuda()
    b = (0.5 * torch.randn(V, generator=g)).cuda()
    tgt = torch.randint(0, V, (R,), generator=g).cuda()
    B = 32
    st = torch.cuda.current_stream().cuda_stream
    row, seq = torch.empty(R, device='cuda'), torch.empty(B, device='cuda')
    nws = torch.empty(int(L.mtl_lm_nll_workspace(R, V)) // 4, device='cuda')
    logits, ws = torch.empty(R, V, device='cuda'), torch.empty(4 << 20, device='cuda')
    lse, hyp, rl, loss = torch.empty(R, device='cuda'), torch.empty(R, dtype=torch.int64, device='cuda'), torch.empty(R, device='cuda'), torch.empty(1, device='cuda')

    def fused():
        assert L.mtl_lm_nll_fwd(st, x.data_ptr(), H, W.data_ptr(), b.data_ptr(), tgt.data_ptr(), R, H, V, B, row.data_ptr(), seq.data_ptr(),
                                nws.data_ptr(), nws.numel() * 4) == 0

    def pair():
        assert L.mtl_gemm_f32_ex(st, 0, 1, R, V, H, 1.0, x.data_ptr(), H, W.data_ptr(), H, logits.data_ptr(), V, b.data_ptr(), None, 0, 0, 1, 1,
                                 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0) == 0
        assert L.mtl_ce_argmax_fwd(st, logits.data_ptr(), tgt.data_ptr(), R, V, V, -1, 0.0, R, None, lse.data_ptr(), hyp.data_ptr(),
                                   rl.data_ptr(), loss.data_ptr()) == 0
    tf, tp = timed(fused, reps), timed(pair, reps)
    flop = 2.0 * R * V * H
    return dict(leg='lm_nll', R=R, H=H, V=V, fused_us=round(tf, 2), gemm_ce_us=round(tp, 2), fused_vs_pair=round(tp / tf, 3),
                fused_fp32_mfma_roof=round(flop / (tf * 1e-6) / FP32_MFMA_ROOF, 3),
                gemm_route=int(L.mtl_gemm_f32_ex_route(R, V, H, 1, 1, 0)))


def evaluate_bench(H, reps):
    import mtl_amd
    from tests import lm_rescore_util as lu
    from tests.test_lm_rescore_gpu import _r0_model
    r0 = lu.load_r0()
    model, args, vocab, (x, lens, y) = _r0_model(r0)
    V = 30011
    torch.manual_seed(0)
    net = mtl_amd.lm.RNNModel('LSTM', V, H, H, 2, 0.2)
    words = ['<oov>', '<eos>'] + r0['words'][2:] + ['v%05d' % i for i in range(V - len(r0['words']))]
    path = os.path.join(tempfile.mkdtemp(), 'lm.pt')
    torch.save(dict(word2idx={w: i for i, w in enumerate(words)}, idx2word=words, ntoken=V, ninp=H, nhid=H, nlayers=2, dropout=0.2,
                    tie_weights=False, model_state_dict=net.state_dict()), path)
    lm = mtl_amd.LM(path, argparse.Namespace(cuda=True))
    xc = x.cuda()
    out = {}
    for name, kw in (('beam', {}), ('beam_lm', dict(lm_rescoring=True, lm=lm, lm_weight=0.6))):
        model.evaluate(xc, lens, y, args, beam_search=True, start_token=vocab.SOS_ID, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            model.evaluate(xc, lens, y, args, beam_search=True, start_token=vocab.SOS_ID, **kw)
        torch.cuda.synchronize()
        out[name + '_ms'] = round((time.perf_counter() - t0) * 1e3 / reps, 2)
    return dict(leg='evaluate', utterances=int(x.shape[0]), lm_V=V, lm_H=H, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    import mtl_amd
    L = mtl_amd._lib.lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))))
    for H in (200, 650):
        print(json.dumps(kernel_bench(L, 256, H, 30011, a.reps)), flush=True)
    for H in (200, 650):
        print(json.dumps(evaluate_bench(H, max(a.reps // 10, 2))), flush=True)


if __name__ == '__main__':
    main()
