"""The narrow convolutions of the large_cnn front-end against the route they replace, and the large_cnn step beside the vgg_cnn step.
usage: python tools/bench_large_cnn.py parent=path.so this=path.so [--no-step]

Kernels, per 8-task launch (8 tasks x 8 utterances) at the north-star extents: 32 -> 32 at 1000 x 161 (pooled) and 32 -> 64 at
500 x 80 (dense), forward / data gradient / weight gradient on the exact split -- `this` build at the narrow shape against the
ZERO-PADDED 64-channel route on the `parent` build (a 64 -> 64 pooled, resp. dense, layer on x3: what ran these shapes before the
narrow kernels existed).  One process, variants alternating, seven samples of 5 launches: median, min, max.  A narrow launch is
counted faster when its median lies below its padded twin's by more than the spread (max - min) of either series.
Step: bench.py's timed span (bench.timed_steps) for 8 tasks at the north-star size on a large_cnn model and, in the same process,
on the vgg_cnn model with conv_x3."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import mtl_amd
from mtl_amd import _lib

USED = ('mtl_conv3x3_wprep_x3', 'mtl_conv3x3_relu_fwd_x3_tb', 'mtl_conv3x3_relu_pool_fwd_x3_tb', 'mtl_conv3x3_dgrad_x3_tb',
        'mtl_conv3x3_wgrad_x3_tb', 'mtl_conv3x3_wgrad_x3_workspace')
libs = {}
for a in sys.argv[1:]:
    if '=' in a:
        n, pth = a.split('=')
        h = ctypes.CDLL(os.path.abspath(pth))
        for name in USED:          # (the parent build does not export what this build added)
            fn = getattr(h, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        libs[n] = h
st = lambda: torch.cuda.current_stream().cuda_stream
dev = 'cuda'
NT, B = 8, 8
REPS, INNER = 7, 5


def operands(kind, T, F, cin, cout, pad):
    """the operands of one layer; pad: the same values inside zero-padded 64-channel tensors"""
    g = torch.Generator(device=dev).manual_seed(7)
    nb = NT * B
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) * 0.05
    x = torch.relu(torch.randn(nb, T, F, cin, device=dev, generator=g))
    bias = torch.randn(cout, device=dev, generator=g) * 0.1
    shape = (nb, T // 2, F // 2, cout) if kind == 'pool' else (nb, T, F, cout)
    dy = torch.randn(shape, device=dev, generator=g)
    am = torch.randint(0, 4, shape, device=dev, generator=g).to(torch.uint8) if kind == 'pool' else None
    if pad:
        ci, co = 64, 64
        wp = torch.zeros(co, ci, 3, 3, device=dev)
        wp[:cout, :cin] = w
        xp = torch.zeros(nb, T, F, ci, device=dev)
        xp[..., :cin] = x
        bp = torch.zeros(co, device=dev)
        bp[:cout] = bias
        dyp = torch.zeros(shape[:3] + (co,), device=dev)
        dyp[..., :cout] = dy
        amp = None
        if am is not None:
            amp = torch.zeros(shape[:3] + (co,), dtype=torch.uint8, device=dev)
            amp[..., :cout] = am
        return wp, xp, bp, dyp, amp, ci, co
    return w, x, bias, dy, am, cin, cout


def case(name, kind, T, F, cin, cout):
    """kind: pool (pooled forward, un-pooling data gradient, pooled weight gradient) | relu (the dense three)"""
    sets = {}
    for n, pad in (('padded', True), ('narrow', False)):
        h = libs['parent' if pad else 'this']
        w, x, bias, dy, am, ci, co = operands(kind, T, F, cin, cout, pad)
        nbytes = 3 * 9 * ci * co * 2
        wf, wd = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert h.mtl_conv3x3_wprep_x3(st(), w.data_ptr(), wf.data_ptr(), wd.data_ptr(), co, ci) == 0
        y = torch.empty(dy.shape, device=dev)
        codes = torch.empty(dy.shape, dtype=torch.uint8, device=dev) if kind == 'pool' else None
        dx = torch.empty(x.shape, device=dev)
        need = h.mtl_conv3x3_wgrad_x3_workspace(B, T, F, ci, co, int(kind == 'pool'))
        ws = torch.empty(need // 4, device=dev)
        dw, db = torch.zeros(NT, co, ci, 3, 3, device=dev), torch.zeros(NT, co, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None
        if kind == 'pool':
            fwd = lambda h=h, a=(p(x), p(wf), p(bias), p(y), p(codes), B, T, F, ci, co, NT, 0, 0, None, 0): h.mtl_conv3x3_relu_pool_fwd_x3_tb(st(), *a)
        else:
            fwd = lambda h=h, a=(p(x), p(wf), p(bias), p(y), B, T, F, ci, co, NT, 0, 0, None, 0): h.mtl_conv3x3_relu_fwd_x3_tb(st(), *a)
        dgrad = lambda h=h, a=(p(dy), p(am), p(wd), p(x), p(dx), B, T, F, ci, co, NT, 0, None, 0): h.mtl_conv3x3_dgrad_x3_tb(st(), *a)
        wgrad = lambda h=h, a=(p(x), p(dy), p(am), p(dw), p(db), p(ws), need, B, T, F, ci, co, NT, 9 * ci * co, co): h.mtl_conv3x3_wgrad_x3_tb(st(), *a)
        sets[n] = dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad, keep=(w, x, bias, dy, am, wf, wd, y, codes, dx, ws, dw, db))
        for k in ('fwd', 'dgrad', 'wgrad'):
            assert sets[n][k]() == 0, (name, n, k)
        torch.cuda.synchronize()
        sets[n]['out'] = (y, dx, dw, db, codes)
    # the two routes compute the same layer: the narrow outputs against the first channels of the padded ones
    yn, dxn, dwn, dbn, cn = sets['narrow']['out']
    yp, dxp, dwp, dbp, cp = sets['padded']['out']
    rel = lambda a_, b_: float((a_.double() - b_.double()).norm() / b_.double().norm().clamp_min(1e-300))
    print('%s narrow vs padded outputs: forward %.1e, data gradient %.1e, weight gradient %.1e, bias gradient %.1e%s'
          % (name, rel(yn, yp[..., :cout]), rel(dxn, dxp[..., :cin]), rel(dwn, dwp[:, :cout, :cin]), rel(dbn, dbp[:, :cout]),
             ', arg-max codes that differ (near-ties of two summation orders): %d of %d' % (int((cn != cp[..., :cout]).sum()), cn.numel())
             if cn is not None else ''), flush=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in ('fwd', 'dgrad', 'wgrad'):
        times = {n: [] for n in sets}
        for rep in range(REPS + 1):
            for n in sets:
                a.record()
                for _ in range(INNER):
                    sets[n][k]()
                b.record()
                torch.cuda.synchronize()
                if rep:
                    times[n].append(a.elapsed_time(b) / INNER)
        med = {n: statistics.median(t) for n, t in times.items()}
        spread = max(max(t) - min(t) for t in times.values())
        for n, t in times.items():
            print('%s %-5s %-6s median %.4f ms  min %.4f  max %.4f  (%s)' % (name, k, n, med[n], min(t), max(t), ' '.join('%.4f' % v for v in t)), flush=True)
        print('%s %-5s narrow / padded = %.3f; narrow faster by more than the spread (%.4f ms): %s'
              % (name, k, med['narrow'] / med['padded'], spread, med['padded'] - med['narrow'] > spread), flush=True)
    del sets
    torch.cuda.empty_cache()


def step():
    """bench.py's timed span, 8 tasks x 8 utterances x 1000 frames x 100 labels: the large_cnn model, then the vgg_cnn model on conv_x3"""
    import contextlib, io
    import bench
    from mtl_amd import dist as mdist
    d = torch.device('cuda', 0)
    for fe in ('large_cnn', 'vgg_cnn', 'large_cnn', 'vgg_cnn'):
        args = bench.make_args(8)
        args.feat_extractor = fe
        vocab = mtl_amd.synthetic_vocab(bench.CFG['vocab_size'])
        torch.manual_seed(123456)
        with contextlib.redirect_stdout(io.StringIO()):
            model = mtl_amd.init_transformer_model(args, vocab, r=bench.CFG['r']).to(d)
        for e in model.engines:
            e.conv_mode, e.conv_x3, e.conv_h2 = 'x3', True, False
        trainer = mtl_amd.TransientTrainer()
        inner, outer = mtl_amd.FlatSGD(model, args.lr), mtl_amd.FlatAdam(model, args.meta_lr)
        model.zero_copy_grad()
        tasks = [bench.ResidentTask(mtl_amd, m, 8, 1000, 100, bench.CFG['vocab_size'], d) for m in range(8)]
        dt, _ = bench.timed_steps(trainer, model, vocab, tasks, mdist.shard_tasks(8, 0, 1), 8, inner, outer, args, 10, 4, mdist, d)
        print('step %-9s (convolutions on x3): %.2f ms per meta-step (10 timed steps after 4)' % (fe, dt / 10 * 1e3), flush=True)
        del model, trainer, inner, outer, tasks
        torch.cuda.empty_cache()


if 'parent' in libs and 'this' in libs:
    case('32->32,1000x161,pooled', 'pool', 1000, 161, 32, 32)
    case('32->64,500x80,dense', 'relu', 500, 80, 32, 64)
if '--no-step' not in sys.argv:
    step()
