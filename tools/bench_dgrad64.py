"""Isolated launches of the 64-channel h2 data gradients at the flagship shapes (8 tasks x 8 utterances), several builds of the library
interleaved in one process.  usage: python tools/bench_dgrad64.py name=path.so [name=path.so ...]   (the first build is the reference of the output comparison)"""
import ctypes, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mtl_amd
from mtl_amd import _lib

libs = []
for a in sys.argv[1:]:
    n, pth = a.split('=')
    h = ctypes.CDLL(os.path.abspath(pth))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    libs.append((n, h))
st = lambda: torch.cuda.current_stream().cuda_stream
dev = 'cuda'
S = 2048
NT, B = 8, 8
REPS, INNER = 7, 5


def case(name, T, F, cin, cout, pooled):
    g = torch.Generator(device=dev).manual_seed(7)
    nb = NT * B
    x = torch.relu(torch.randn(nb, T, F, cin, device=dev, generator=g))
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) * 0.05
    L0 = libs[0][1]
    nbytes = L0.mtl_conv3x3_wprep_h2_bytes(cout, cin)
    w2f, w2d = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert L0.mtl_conv3x3_wprep_h2(st(), w.data_ptr(), w2f.data_ptr(), w2d.data_ptr(), cout, cin) == 0
    if pooled:
        dy = torch.randn(nb, T // 2, F // 2, cout, device=dev, generator=g)
        am = torch.randint(0, 4, dy.shape, device=dev, generator=g).to(torch.uint8)
        amp = am.data_ptr()
    else:
        dy = torch.randn(nb, T, F, cout, device=dev, generator=g)
        dy = dy * (torch.rand(dy.shape, device=dev, generator=g) > 0.5)
        amp = None
    ady = torch.stack([dy[t * B:(t + 1) * B].abs().max().reshape(1).repeat(S) for t in range(NT)]).contiguous()
    outs, times = {}, {n: [] for n, _ in libs}
    for n, h in libs:
        dx = torch.full_like(x, float('nan'))
        adx = torch.zeros(NT, S, device=dev)
        rc = h.mtl_conv3x3_dgrad_h2_tb(st(), dy.data_ptr(), ady.data_ptr(), amp, w2d.data_ptr(), x.data_ptr(), dx.data_ptr(), adx.data_ptr(),
                                       B, T, F, cin, cout, NT, 0, S, S, None, 0)
        assert rc == 0, (n, rc)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(dx).any()), n
        outs[n] = (dx[::9].clone(), adx.view(NT, -1, 32)[:, :, 0].max(1)[0].clone(), float(dx.abs().max()))
        del dx
    ref = outs[libs[0][0]]
    for n, _ in libs[1:]:
        d = (outs[n][0] - ref[0]).abs().max().item()
        print('%s %s vs %s: max|diff| %.3e of max|dx| %.3e, bit-identical %s, bounds equal %s' % (
            name, n, libs[0][0], d, ref[2], torch.equal(outs[n][0], ref[0]), torch.equal(outs[n][1], ref[1])), flush=True)
    dx = torch.empty_like(x)
    adx = torch.zeros(NT, S, device=dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS + 1):
        for n, h in libs:
            a.record()
            for _ in range(INNER):
                h.mtl_conv3x3_dgrad_h2_tb(st(), dy.data_ptr(), ady.data_ptr(), amp, w2d.data_ptr(), x.data_ptr(), dx.data_ptr(), adx.data_ptr(),
                                          B, T, F, cin, cout, NT, 0, S, S, None, 0)
            b.record()
            torch.cuda.synchronize()
            if rep:
                times[n].append(a.elapsed_time(b) / INNER)
    for n, _ in libs:
        t = times[n]
        print('%s %-8s median %.4f ms  min %.4f  max %.4f  (%s)' % (name, n, statistics.median(t), min(t), max(t), ' '.join('%.4f' % v for v in t)), flush=True)


case('conv2_dgrad(64->64,pooled,1000x161)', 1000, 161, 64, 64, True)
case('conv5_dgrad(64->128,dense,500x80)', 500, 80, 64, 128, False)
case('conv7_dgrad(128->128,pooled,500x80;control)', 500, 80, 128, 128, True)
