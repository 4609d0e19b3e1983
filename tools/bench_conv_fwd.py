"""Isolated 8-task launches of the h2 forwards / pool forwards and of conv7's data gradient at the flagship shapes (8 tasks x 8 utterances,
1000 x 161 -> 500 x 80), several builds of the library interleaved in one process; conv5's data gradient runs as an unchanged-code control.
usage: python tools/bench_conv_fwd.py name=path.so [name=path.so ...]   (the first build is the reference of the output comparison:
values, arg-max codes and bounds must be equal bit for bit).  7 samples of 5 launches per build and case: median, min, max."""
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
ok_all = True


def amax(t):
    return torch.stack([t[k * B:(k + 1) * B].abs().max().reshape(1).repeat(S) for k in range(NT)]).contiguous()


def case(name, kind, T, F, cin, cout):
    """kind: relu | pool | dgrad_p | dgrad_d; cin / cout are the forward convolution's"""
    global ok_all
    g = torch.Generator(device=dev).manual_seed(7)
    nb = NT * B
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) * 0.05
    L0 = libs[0][1]
    nbytes = L0.mtl_conv3x3_wprep_h2_bytes(cout, cin)
    w2f, w2d = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert L0.mtl_conv3x3_wprep_h2(st(), w.data_ptr(), w2f.data_ptr(), w2d.data_ptr(), cout, cin) == 0
    x = torch.relu(torch.randn(nb, T, F, cin, device=dev, generator=g))
    am = None
    if kind in ('relu', 'pool'):
        bias = torch.randn(cout, device=dev, generator=g) * 0.1
        ain = amax(x)
        oshape = (nb, T // 2, F // 2, cout) if kind == 'pool' else (nb, T, F, cout)
    else:
        if kind == 'dgrad_p':
            dy = torch.randn(nb, T // 2, F // 2, cout, device=dev, generator=g)
            am = torch.randint(0, 4, dy.shape, device=dev, generator=g).to(torch.uint8)
        else:
            dy = torch.randn(nb, T, F, cout, device=dev, generator=g)
            dy = dy * (torch.rand(dy.shape, device=dev, generator=g) > 0.5)
        ain = amax(dy)
        oshape = x.shape

    def launch(h, out, codes, aout):
        if kind == 'relu':
            return h.mtl_conv3x3_relu_fwd_h2_tb(st(), x.data_ptr(), ain.data_ptr(), w2f.data_ptr(), bias.data_ptr(), out.data_ptr(), aout.data_ptr(),
                                                B, T, F, cin, cout, NT, 0, 0, S, S, None, 0)
        if kind == 'pool':
            return h.mtl_conv3x3_relu_pool_fwd_h2_tb(st(), x.data_ptr(), ain.data_ptr(), w2f.data_ptr(), bias.data_ptr(), out.data_ptr(), codes.data_ptr(),
                                                     aout.data_ptr(), B, T, F, cin, cout, NT, 0, 0, S, S, None, 0)
        return h.mtl_conv3x3_dgrad_h2_tb(st(), dy.data_ptr(), ain.data_ptr(), am.data_ptr() if am is not None else None, w2d.data_ptr(), x.data_ptr(),
                                         out.data_ptr(), aout.data_ptr(), B, T, F, cin, cout, NT, 0, S, S, None, 0)

    ref = None
    for n, h in libs:
        out = torch.full(oshape, float('nan'), device=dev)
        codes = torch.full(oshape, 0xEE, dtype=torch.uint8, device=dev) if kind == 'pool' else None
        aout = torch.zeros(NT, S, device=dev)
        rc = launch(h, out, codes, aout)
        assert rc == 0, (n, rc)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()), n
        bound = aout.view(NT, -1, 32)[:, :, 0].max(1)[0].clone()
        if ref is None:
            ref = (out, codes, bound, n)
        else:
            same = (torch.equal(out.view(torch.int32), ref[0].view(torch.int32)), codes is None or torch.equal(codes, ref[1]), torch.equal(bound, ref[2]))
            ok_all = ok_all and all(same)
            print('%s %s vs %s: values bit-identical %s, arg-max codes equal %s, bounds equal %s' % (name, n, ref[3], same[0], same[1], same[2]), flush=True)
            del out, codes
    del ref
    out = torch.empty(oshape, device=dev)
    codes = torch.empty(oshape, dtype=torch.uint8, device=dev) if kind == 'pool' else None
    aout = torch.zeros(NT, S, device=dev)
    times = {n: [] for n, _ in libs}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS + 1):
        for n, h in libs:
            a.record()
            for _ in range(INNER):
                launch(h, out, codes, aout)
            b.record()
            torch.cuda.synchronize()
            if rep:
                times[n].append(a.elapsed_time(b) / INNER)
    for n, _ in libs:
        t = times[n]
        print('%s %-8s median %.4f ms  min %.4f  max %.4f  (%s)' % (name, n, statistics.median(t), min(t), max(t), ' '.join('%.4f' % v for v in t)), flush=True)


case('conv2_fwd_pool(64->64,1000x161)', 'pool', 1000, 161, 64, 64)
case('conv2_fwd_no_pool(64->64,1000x161;not on the flagship step)', 'relu', 1000, 161, 64, 64)
case('conv5_fwd(64->128,500x80)', 'relu', 500, 80, 64, 128)
case('conv7_fwd_pool(128->128,500x80)', 'pool', 500, 80, 128, 128)
case('conv7_dgrad(128->128,pooled,500x80)', 'dgrad_p', 500, 80, 128, 128)
case('conv5_dgrad(64->128,dense,500x80;control)', 'dgrad_d', 500, 80, 64, 128)
print('outputs equal to the reference build in every case: %s' % ok_all, flush=True)
sys.exit(0 if ok_all else 1)
