"""mtl_ffn_lr_mid_fwd (csrc/mtl_ffn_lr.hip: h = relu(a . B1^T + b1), c = h . A2^T in one streamed kernel) through the C ABI against fp64
torch, at the smallest shapes at which it can go wrong: rows across the wave (16) and workgroup (64) row blocks, r at 100 / 36 / 128
(7, 3 and 8 column accumulators; 4, 2 and 4 contraction steps), inner at one chunk (64), a ragged chunk (72), chunks plus a tail (200)
and the real size (512), one and three tasks with their own and with shared weights, padded lda / ldc, h stored and not stored.

Accuracy is measured against the route the engine takes without the kernel -- mtl_gemm_f32_ex with bias + ReLU, then a second call --
on the same inputs: the fused result's relative error against fp64 may be at most twice that route's (the summation order differs,
nothing else).  Sign decisions of the stored h must be those of the fp64 pre-activation wherever it is farther from zero than the
bound ERR_Z * (|a| . |B1|^T + |b1|): a product of K <= 128 terms accumulated in fp32 is off by at most K 2^-24 of the sum of the terms'
magnitudes, the dropped terms of the bf16 triples add 2^-22, the bias add one rounding: (128 + 4 + 1) 2^-24 = 7.9e-6 < ERR_Z = 1e-5."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_Z = 1e-5
SENTINEL = 7777.0
# rows, r, inner, tasks, per-task weights, extra lda, extra ldc
CASES = [(1, 100, 64, 1, False, 0, 0),
         (15, 36, 72, 3, True, 0, 0),
         (64, 128, 200, 1, False, 0, 0),
         (65, 100, 512, 3, False, 0, 0),
         (130, 100, 200, 3, True, 28, 12),
         (130, 36, 72, 1, False, 4, 92),
         (65, 128, 64, 3, True, 0, 4),
         (15, 100, 512, 1, False, 12, 0)]


def inputs(rows, r, inner, tasks, own, seed):
    """seeded fp32 inputs: a ~ N(0, 1), B1 ~ N(0, 1 / r), b1 ~ N(0, 1 / 4), A2 ~ N(0, 1 / inner): pre-activations of unit scale"""
    g = torch.Generator().manual_seed(seed)
    nw = tasks if own else 1
    a = torch.randn(tasks, rows, r, generator=g)
    B1 = torch.randn(nw, inner, r, generator=g) / r ** 0.5
    b1 = torch.randn(nw, inner, generator=g) * 0.5
    A2 = torch.randn(nw, r, inner, generator=g) / inner ** 0.5
    return a, B1, b1, A2


def reference(a, B1, b1, A2):
    """fp64: pre-activation z, its error band, h, c -- per task (shared weights broadcast)"""
    a64, B64, b64, A64 = (t.double() for t in (a, B1, b1, A2))
    z = a64 @ B64.transpose(1, 2) + b64.unsqueeze(1)
    band = ERR_Z * (a64.abs() @ B64.abs().transpose(1, 2) + b64.abs().unsqueeze(1))
    h = z.clamp_min(0)
    return z, band, h, h @ A64.transpose(1, 2)


def rel(x, ref):
    return float((x.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'rows%d-r%d-inner%d-tasks%d-%s-lda+%d-ldc+%d' % (c[:4] + ('own' if c[4] else 'shared',) + c[5:]))
def test_inputs_leave_few_preactivations_inside_the_error_band(case):
    """(CPU arithmetic only) at most 1e-3 of the fp64 pre-activations lie where a correct kernel may decide the ReLU either way"""
    rows, r, inner, tasks, own, _, _ = case
    z, band, _, _ = reference(*inputs(rows, r, inner, tasks, own, seed=1000 + rows + r + inner))
    assert float((z.abs() <= band).double().mean()) <= 1e-3


@functools.lru_cache(maxsize=None)
def run(case):
    import mtl_amd
    L = mtl_amd._lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows, r, inner, tasks, own, xa, xc = case
    a, B1, b1, A2 = inputs(rows, r, inner, tasks, own, seed=1000 + rows + r + inner)
    z, band, h64, c64 = reference(a, B1, b1, A2)
    lda, ldc, pad = r + xa, r + xc, 3                       # `pad` rows behind every task's rows in the output buffers
    da = torch.full((tasks, rows, lda), SENTINEL, device='cuda')
    da[:, :, :r] = a.cuda()
    dB1, db1, dA2 = B1.cuda().contiguous(), b1.cuda().contiguous(), A2.cuda().contiguous()
    # one flat weight buffer per task, as in theta: B1 | b1 | A2 at a common task stride
    per = inner * r + inner + r * inner
    W = torch.empty(B1.shape[0], per, device='cuda')
    W[:, :inner * r], W[:, inner * r:inner * r + inner], W[:, inner * r + inner:] = dB1.flatten(1), db1, dA2.flatten(1)
    sWt = per if own else 0
    assert per % 4 == 0
    pB1, pb1, pA2 = W.data_ptr(), W.data_ptr() + 4 * inner * r, W.data_ptr() + 4 * (inner * r + inner)

    def fused(store_h):
        h = torch.full((tasks, rows + pad, inner), SENTINEL, device='cuda')
        c = torch.full((tasks, rows + pad, ldc), SENTINEL, device='cuda')
        rc = L.mtl_ffn_lr_mid_fwd(st, da.data_ptr(), lda, pB1, pb1, pA2, h.data_ptr() if store_h else None, c.data_ptr(), ldc, rows, r, inner,
                                  tasks, rows * lda, sWt, (rows + pad) * inner, (rows + pad) * ldc)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return h.cpu(), c.cpu()
    h1, c1 = fused(True)
    h1b, c1b = fused(True)
    h0, c0 = fused(False)
    # the two-call route on the same inputs (code from before this kernel): one task at a time
    ws = torch.empty(1 << 20, device='cuda')
    h2 = torch.empty(tasks, rows, inner, device='cuda')
    c2 = torch.empty(tasks, rows, r, device='cuda')
    for t in range(tasks):
        w = 4 * t * sWt
        tail = (1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None, 0, ws.data_ptr(), ws.numel() * 4, 0, 0)
        assert L.mtl_gemm_f32_ex(st, 0, 1, rows, inner, r, 1.0, da[t].data_ptr(), lda, pB1 + w, r, h2[t].data_ptr(), inner, pb1 + w, None, 0, 1,
                                 *tail) == 0
        assert L.mtl_gemm_f32_ex(st, 0, 1, rows, r, inner, 1.0, h2[t].data_ptr(), inner, pA2 + w, inner, c2[t].data_ptr(), r, None, None, 0, 0,
                                 *tail) == 0
    torch.cuda.synchronize()
    return dict(z=z, band=band, h64=h64, c64=c64, h1=h1, c1=c1, h1b=h1b, c1b=c1b, h0=h0, c0=c0, h2=h2.cpu(), c2=c2.cpu())


def test_supported_answers_as_documented():
    import mtl_amd
    L = mtl_amd._lib.lib()
    for r in range(0, 140):
        for inner in (0, 2, 4, 64, 70, 72, 512, 2048):
            assert L.mtl_ffn_lr_mid_supported(r, inner) == int(4 <= r <= 128 and r % 4 == 0 and inner >= 4 and inner % 4 == 0), (r, inner)
    x = torch.zeros(64, device='cuda')
    st, p = torch.cuda.current_stream().cuda_stream, x.data_ptr()
    assert L.mtl_ffn_lr_mid_fwd(st, p, 132, p, p, p, None, p, 132, 1, 132, 64, 1, 0, 0, 0, 0) == -22       # r beyond 128
    assert L.mtl_ffn_lr_mid_fwd(st, p, 100, p, p, p, None, p, 100, 1, 100, 70, 1, 0, 0, 0, 0) == -22       # inner not a multiple of 4
    assert L.mtl_ffn_lr_mid_fwd(st, p, 98, p, p, p, None, p, 100, 1, 100, 64, 1, 0, 0, 0, 0) == -22        # lda below r
    assert L.mtl_ffn_lr_mid_fwd(st, p, 100, p, p, p, None, p, 100, 0, 100, 64, 1, 0, 0, 0, 0) == -22       # no rows


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'rows%d-r%d-inner%d-tasks%d-%s-lda+%d-ldc+%d' % (c[:4] + ('own' if c[4] else 'shared',) + c[5:]))
def test_fused_middle(case):
    rows, r, inner, tasks, own, xa, xc = case
    R = run(case)
    h1, c1 = R['h1'], R['c1']
    # nothing outside the results is written
    assert bool((h1[:, rows:] == SENTINEL).all()) and bool((c1[:, rows:] == SENTINEL).all()) and bool((c1[:, :, r:] == SENTINEL).all())
    assert bool((R['h0'] == SENTINEL).all()), 'h = NULL, yet the h buffer was written'
    # h stored or not: the same c bit for bit; two runs: the same bits
    assert torch.equal(c1, R['c0']) and torch.equal(c1, R['c1b']) and torch.equal(h1, R['h1b'])
    h, c = h1[:, :rows], c1[:, :rows, :r]
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all())
    # ReLU decisions against the fp64 pre-activation outside the error band
    z, band = R['z'], R['band']
    sure = z.abs() > band
    wrong = ((h > 0) != (z > 0)) & sure
    print('%s: %d of %d pre-activations inside the band (decided either way), %d decisions wrong outside it'
          % (case, int((~sure).sum()), z.numel(), int(wrong.sum())))
    assert int(wrong.sum()) == 0
    assert bool((h >= 0).all())
    # accuracy: at most twice the two-call route's error against fp64
    eh, eh2 = rel(h, R['h64']), rel(R['h2'], R['h64'])
    ec, ec2 = rel(c, R['c64']), rel(R['c2'], R['c64'])
    print('%s: rel err vs fp64  h fused %.3e two-call %.3e   c fused %.3e two-call %.3e' % (case, eh, eh2, ec, ec2))
    assert eh <= 2 * eh2 and ec <= 2 * ec2, (eh, eh2, ec, ec2)
