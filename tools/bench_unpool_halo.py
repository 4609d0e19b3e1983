"""A/B of the un-pooling h2 data gradients (conv2: 64 -> 64, conv7: 128 -> 128) against the parent commit's build: isolated 8-task launches at the
flagship shapes (8 tasks x 8 utterances), the builds alternating in one process, 7 samples of 5 launches each; conv5's dense data gradient
(code the halo change does not touch) is the control.  Outputs and output bounds are compared bit for bit with the parent's.
usage: python tools/bench_unpool_halo.py parent=<parent commit's libmtl_hip.so> this=<this build> [name=path.so ...]
Verdict per kernel: `gain` only if this build's median lies below the parent's median by more than the parent's own least-to-largest spread."""
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
assert len(libs) >= 2 and libs[0][0] == 'parent', __doc__
st = lambda: torch.cuda.current_stream().cuda_stream
dev = 'cuda'
S = 2048
NT, B = 8, 8
REPS, INNER = 7, 5
all_equal = True


def case(name, T, F, cin, cout, pooled, control):
    global all_equal
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

    def run(h, dx, adx):
        return h.mtl_conv3x3_dgrad_h2_tb(st(), dy.data_ptr(), ady.data_ptr(), amp, w2d.data_ptr(), x.data_ptr(), dx.data_ptr(), adx.data_ptr(),
                                         B, T, F, cin, cout, NT, 0, S, S, None, 0)

    ref = None
    for n, h in libs:
        dx = torch.full_like(x, float('nan'))
        adx = torch.zeros(NT, S, device=dev)
        rc = run(h, dx, adx)
        assert rc == 0, (n, rc)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(dx).any()), n
        if ref is None:
            ref = (dx, adx)
            continue
        same = torch.equal(dx.view(torch.int32), ref[0].view(torch.int32))
        all_equal = all_equal and same
        print('%s %s vs parent: max|diff| %.3e of max|dx| %.3e, bit-identical %s, bounds equal %s' % (
            name, n, (dx - ref[0]).abs().max().item(), ref[0].abs().max().item(), same, torch.equal(adx, ref[1])), flush=True)
        del dx
    dx, adx = ref
    times = {n: [] for n, _ in libs}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS + 1):                    # (the first round warms up)
        for n, h in libs:
            a.record()
            for _ in range(INNER):
                run(h, dx, adx)
            b.record()
            torch.cuda.synchronize()
            if rep:
                times[n].append(a.elapsed_time(b) / INNER)
    for n, _ in libs:
        t = times[n]
        print('%s %-8s median %.4f ms  min %.4f  max %.4f  (%s)' % (name, n, statistics.median(t), min(t), max(t), ' '.join('%.4f' % v for v in t)), flush=True)
    tp = times['parent']
    mp, spread = statistics.median(tp), max(tp) - min(tp)
    for n, _ in libs[1:]:
        d = mp - statistics.median(times[n])
        if control:
            verdict = 'control inside the spread' if abs(d) <= spread else 'CONTROL OUTSIDE THE SPREAD'
        else:
            verdict = 'gain' if d > spread else 'no gain'
        print('%s %-8s parent median - median %+.4f ms (%+.2f %%), parent spread %.4f ms: %s' % (name, n, d, 100.0 * d / mp, spread, verdict), flush=True)


case('conv2_dgrad(64->64,pooled,1000x161)', 1000, 161, 64, 64, True, False)
case('conv7_dgrad(128->128,pooled,500x80)', 500, 80, 128, 128, True, False)
case('conv5_dgrad(64->128,dense,500x80;control)', 500, 80, 64, 128, False, True)
print('outputs bit-identical with the parent: %s' % all_equal)
sys.exit(0 if all_equal else 1)
