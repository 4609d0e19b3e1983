"""The split-bf16 ("x3") kernels against fp64 at bounds that tell six piece products from five.

mtl_attn_fwd / mtl_attn_bwd (head size 64), the mtl_conv3x3_*_x3 family (single-task and _tb) and the x3 GEMM engine are compared
with fp64 computed on the CPU from the identical fp32 inputs.  The bound of every case comes from the CPU emulation in
tests/x3_emul.py alone -- half of what the cheapest dropped second-order term costs (random inputs), an eighth of it (probes whose
leading piece product cancels) -- and tests/test_x3_emulation.py shows without a GPU that each bound separates six terms from
five.  Every launch is made twice and must repeat bit for bit.  Each test prints the kernel's error, the bound and the ratio to
torch fp32 on the CPU (-s); the bounds and the errors measured on an MI355X: DESIGN.md, "x3 accuracy against fp64"."""
import pytest
import torch
import torch.nn.functional as F

from tests import x3_emul as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


@pytest.fixture
def x3_forced(L):
    """every eligible product of mtl_gemm_f32_ex goes to the bf16-split engine (threshold 1 tile) for the duration of a test"""
    old = L.mtl_gemm_x3_min_tiles(1)
    yield
    L.mtl_gemm_x3_min_tiles(old)


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(t):
    return t.cuda().contiguous()


def report(what, errs, bound, f32):
    """print the measured errors beside the bound and torch fp32, then THE assertion (x3_emul.check)"""
    for n, e in errs.items():
        print('\nx3-precision %-40s %-5s kernel %.3e   bound %.3e (kernel / bound %.2f)   torch fp32 %.3e (kernel / fp32 %.2f)' % (
            what, n, e, bound, e / bound, f32[n], e / f32[n]), end='')
    E.check(errs, bound, what)


# ------------------------------------------------------------------------------------------------ attention
def run_attention(L, inp, strided):
    """mtl_attn_fwd then mtl_attn_bwd on the case's inputs -> O, lse, dq, dk, dv on the CPU in (B, T, H d) layout.
    strided: q / k / v are the column blocks of one (rows, 3 H d) matrix, dO a column block of a (rows, 2 H d) one; O, dq, dk and
    dv each go into one block of a buffer of their own that is 2 H d or 3 H d wide and filled with NaN: afterwards the head
    columns hold no NaN and every other column still does."""
    B, H, Tq, Tk, d = inp['B'], inp['H'], inp['Tq'], inp['Tk'], E.D_HEAD
    hd = H * d
    g = torch.Generator().manual_seed(99)
    if strided:
        assert Tq == Tk
        qkv = torch.randn(B, Tq, 3 * hd, generator=g)
        qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:] = inp['q'], inp['k'], inp['v']
        dOw = torch.randn(B, Tq, 2 * hd, generator=g)
        dOw[..., hd:] = inp['dO']
        qkv, dOw = dev(qkv), dev(dOw)
        q_p, k_p, v_p, dO_p = qkv.data_ptr(), qkv.data_ptr() + 4 * hd, qkv.data_ptr() + 8 * hd, dOw.data_ptr() + 4 * hd
        ldq = ldk = ldv = 3 * hd
        ldo = 2 * hd
    else:
        dq_, dk_, dv_, ddO = dev(inp['q']), dev(inp['k']), dev(inp['v']), dev(inp['dO'])
        q_p, k_p, v_p, dO_p = dq_.data_ptr(), dk_.data_ptr(), dv_.data_ptr(), ddO.data_ptr()
        ldq = ldk = ldv = ldo = hd
    klen = dev(torch.tensor(inp['klens'], dtype=torch.int32)) if inp['klens'] is not None else None
    keep = dev(inp['keep']) if inp['keep'] is not None else None
    klen_p = klen.data_ptr() if klen is not None else None
    keep_p = keep.data_ptr() if keep is not None else None
    scale, pscale, ldm, causal = inp['scale'], inp['pscale'], inp['ldm'], inp['causal']
    nan = float('nan')
    if strided:
        Ow = torch.full((B, Tq, 2 * hd), nan).cuda()               # O in the FIRST block (dO sits in the second block of its matrix)
        # dq in the middle block of a 3 H d row, dk in the last block of a 2 H d row, dv in the first block of a 3 H d row
        Gq, Gk, Gv = torch.full((B, Tq, 3 * hd), nan).cuda(), torch.full((B, Tk, 2 * hd), nan).cuda(), torch.full((B, Tk, 3 * hd), nan).cuda()
        O_p, gq_p, gk_p, gv_p = Ow.data_ptr(), Gq.data_ptr() + 4 * hd, Gk.data_ptr() + 4 * hd, Gv.data_ptr()
        lddq, lddk, lddv = 3 * hd, 2 * hd, 3 * hd
    else:
        Ow = torch.full((B, Tq, hd), nan).cuda()
        gq, gk, gv = torch.full((B, Tq, hd), nan).cuda(), torch.full((B, Tk, hd), nan).cuda(), torch.full((B, Tk, hd), nan).cuda()
        O_p, gq_p, gk_p, gv_p = Ow.data_ptr(), gq.data_ptr(), gk.data_ptr(), gv.data_ptr()
        lddq = lddk = lddv = hd
    lse = torch.empty(B, H, Tq).cuda()
    delta = torch.empty(B * H * Tq).cuda()
    assert L.mtl_attn_fwd(st(), q_p, k_p, v_p, ldq, ldk, ldv, klen_p, causal, scale, B, H, Tq, Tk, d, d, keep_p, ldm, pscale, O_p, ldo,
                          lse.data_ptr()) == 0
    if strided:     # the backward reads O and dO with ONE row stride: both are blocks of (rows, 2 H d) matrices
        assert bool(torch.isnan(Ow[..., hd:]).all()) and not bool(torch.isnan(Ow[..., :hd]).any())
    assert L.mtl_attn_bwd(st(), q_p, k_p, v_p, ldq, ldk, ldv, klen_p, causal, scale, B, H, Tq, Tk, d, d, keep_p, ldm, pscale, O_p, dO_p,
                          ldo, lse.data_ptr(), delta.data_ptr(), gq_p, gk_p, gv_p, lddq, lddk, lddv) == 0
    torch.cuda.synchronize()
    if strided:
        Ow, Gq, Gk, Gv = Ow.cpu(), Gq.cpu(), Gk.cpu(), Gv.cpu()
        out = dict(O=Ow[..., :hd], lse=lse.cpu(), dq=Gq[..., hd:2 * hd], dk=Gk[..., hd:], dv=Gv[..., :hd])
        guards = dict(O=[Ow[..., hd:]], dq=[Gq[..., :hd], Gq[..., 2 * hd:]], dk=[Gk[..., :hd]], dv=[Gv[..., hd:]])
        for n, gs in guards.items():
            assert not bool(torch.isnan(out[n]).any()), 'NaN left in the head columns of ' + n
            assert all(bool(torch.isnan(gd).all()) for gd in gs), 'a store of %s went outside its head columns' % n
        return out
    return dict(O=Ow.cpu(), lse=lse.cpu(), dq=gq.cpu(), dk=gk.cpu(), dv=gv.cpu())


def attention_case(L, name, strided=False):
    inp, rep, ref = E.attn_inputs(name), E.attn_report(name), E.attn_reference(name)
    outs = [run_attention(L, inp, strided) for _ in range(2)]
    for n in outs[0]:
        assert not bool(torch.isnan(outs[0][n]).any()), n
        assert torch.equal(outs[0][n], outs[1][n]), n
    errs = E.attn_errors(outs[0], ref)
    return rep, errs


@pytest.mark.parametrize('name', sorted(E.ATTN_CASES))
def test_attention_keeps_all_six_terms_of_every_product(L, name):
    """random N(0,1) inputs: O, dq, dk, dv within B (relative L2) and lse within B max|lse| of fp64, B = half of the cheapest of the
    18 (product, term) drops of the emulation.  The cases: ragged causal and cross attention over three key tiles, exactly one
    full tile, dropout on the probabilities, more than 1024 workgroups (the backward's two-launch form; B from a one-batch,
    two-head slice of the same inputs), and q / k / v / dO / O / gradients as column blocks of wider matrices (row stride
    3 H d, as the decode session and a fused q|k|v projection store them)."""
    rep, errs = attention_case(L, name, strided=E.ATTN_CASES[name][8])
    report('attention ' + name, errs, rep['bound'], rep['f32'])


@pytest.mark.parametrize('name', sorted(E.ATTN_PROBES))
def test_attention_probe_weighs_a_second_order_term_at_2_to_the_minus_9(L, name):
    """Q K^T and dO V^T take both operands from outside: one constant-lead, the other antisymmetric along the head dimension, so
    the product is carried by a first-order cross term and a missing a1 b1 / a2 b0 / a0 b2 costs 2^-9 of it.  Probed outputs
    within Bp = 1/8 of the cheaper targeted drop."""
    rep, errs = attention_case(L, name)
    report('attention probe ' + name, {o: errs[o] for o in rep['outputs']}, rep['bound'], rep['f32'])


# ------------------------------------------------------------------------------------------------ 3 x 3 convolutions
def wprep(L, w, Cin, Cout):
    """w (n, Cout, Cin, 3, 3) on the device -> the forward and data-gradient bf16 triples of each"""
    n = w.shape[0]
    w3f = torch.empty(n, 3 * 9 * Cin * Cout, dtype=torch.bfloat16).cuda()
    w3d = torch.empty(n, 3 * 9 * Cin * Cout, dtype=torch.bfloat16).cuda()
    for k in range(n):
        assert L.mtl_conv3x3_wprep_x3(st(), w[k].data_ptr(), w3f[k].data_ptr(), w3d[k].data_ptr(), Cout, Cin) == 0
    return w3f, w3d


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    return a


def fp64_gradients(x, w, dy_full):
    """data and weight gradient of conv2d(x, w, padding=1) for the full-resolution output gradient dy_full, torch.nn.functional in fp64"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, padding=1).backward(dy_full.double())
    return xr.grad * (x > 0), wr.grad


def check_argmax(am, ref, T, tol):
    """the kernel's arg-max codes pick a maximum of the fp64 window: exact, or a near-tie within the forward's rounding"""
    B, C, Fp, Tp = am.shape
    f = torch.arange(Fp).view(1, 1, Fp, 1) * 2 + (am.long() >> 1)
    t = torch.arange(Tp).view(1, 1, 1, Tp) * 2 + (am.long() & 1)
    chosen = ref['y'].reshape(B, C, -1).gather(2, (f * T + t).view(B, C, -1)).view(B, C, Fp, Tp)
    assert float((ref['p'] - chosen).max()) <= tol * float(ref['y'].max())
    assert float((am != E.codes_of(ref['idx'], T)).float().mean()) < 1e-3


def conv_case(L, shape, tasks):
    """the four x3 convolution kernels (forward, fused pool, data gradient dense + pooled, weight gradient dense + pooled) on
    `tasks` stacked batches with per-task weights: single-task entry points for tasks = 1, the _tb ones otherwise"""
    Cin, Cout, B, T, Fq = shape
    inp, refs = E.conv_inputs(shape, tasks), E.conv_reference(shape, tasks)
    dense = [E.conv_report(shape, tasks, False, t) for t in range(tasks)]      # every task has its own bounds
    pooled = [E.conv_report(shape, tasks, True, t) for t in range(tasks)]
    tb = tasks > 1
    Tp, Fp = T // 2, Fq // 2
    xn = dev(torch.cat([E.nhwc(inp['x'][t]) for t in range(tasks)]))                    # (tasks B, T, F, Cin)
    w, b = dev(inp['w']), dev(inp['b'])
    w3f, w3d = wprep(L, w, Cin, Cout)
    sW, sB = w3f[0].numel() * 2, Cout
    what = 'conv %s%s ' % (shape, ' x %d tasks' % tasks if tb else '')

    def per_task(t_nhwc):           # (tasks B, T', F', C) -> per task, reference layout
        return [E.nhwc(t_nhwc[t * B:(t + 1) * B]) for t in range(tasks)]

    def fwd():
        y = torch.full((tasks * B, T, Fq, Cout), float('nan')).cuda()
        if tb:
            assert L.mtl_conv3x3_relu_fwd_x3_tb(st(), xn.data_ptr(), w3f.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, Fq, Cin, Cout, tasks,
                                                sW, sB, None, 0) == 0
        else:
            assert L.mtl_conv3x3_relu_fwd_x3(st(), xn.data_ptr(), w3f.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, Fq, Cin, Cout) == 0
        return [y.cpu()]

    def pool():
        p = torch.full((tasks * B, Tp, Fp, Cout), float('nan')).cuda()
        am = torch.full((tasks * B, Tp, Fp, Cout), 9, dtype=torch.uint8).cuda()
        if tb:
            assert L.mtl_conv3x3_relu_pool_fwd_x3_tb(st(), xn.data_ptr(), w3f.data_ptr(), b.data_ptr(), p.data_ptr(), am.data_ptr(), B, T, Fq,
                                                     Cin, Cout, tasks, sW, sB, None, 0) == 0
        else:
            assert L.mtl_conv3x3_relu_pool_fwd_x3(st(), xn.data_ptr(), w3f.data_ptr(), b.data_ptr(), p.data_ptr(), am.data_ptr(), B, T, Fq,
                                                  Cin, Cout) == 0
        return [p.cpu(), am.cpu()]
    y = per_task(twice(fwd)[0])
    p_all, am_all = twice(pool)
    p, am, am_dev = per_task(p_all), per_task(am_all), dev(am_all)
    for t in range(tasks):
        report(what + 'forward task %d' % t, {'fwd': E.rel(y[t], refs[t]['y'])}, dense[t]['fwd']['bound'], {'fwd': dense[t]['fwd']['f32']})
        report(what + 'pooled forward task %d' % t, {'fwd': E.rel(p[t], refs[t]['p'])}, pooled[t]['fwd']['bound'], {'fwd': pooled[t]['fwd']['f32']})
        check_argmax(am[t], refs[t], T, pooled[t]['fwd']['bound'])

    for is_pooled, reps in ((False, dense), (True, pooled)):
        if is_pooled:
            dyn = dev(torch.cat([E.nhwc(refs[t]['dpg']) for t in range(tasks)]))       # gradient of the pooled output, gated by p > 0
            full = [E.scatter_pooled(refs[t]['dpg'], am[t], Fq, T) for t in range(tasks)]
            am_p = am_dev.data_ptr()
        else:
            dyn = dev(torch.cat([E.nhwc(refs[t]['dyg']) for t in range(tasks)]))       # gradient of the dense output, gated by y > 0
            full = [refs[t]['dyg'] for t in range(tasks)]
            am_p = None
        need = L.mtl_conv3x3_wgrad_x3_workspace(B, T, Fq, Cin, Cout, 1 if is_pooled else 0)
        ws = torch.empty(need // 4 + 64).cuda()

        def dgrad():
            dx = torch.full((tasks * B, T, Fq, Cin), float('nan')).cuda()
            if tb:
                assert L.mtl_conv3x3_dgrad_x3_tb(st(), dyn.data_ptr(), am_p, w3d.data_ptr(), xn.data_ptr(), dx.data_ptr(), B, T, Fq, Cin, Cout,
                                                 tasks, sW, None, 0) == 0
            else:
                assert L.mtl_conv3x3_dgrad_x3(st(), dyn.data_ptr(), am_p, w3d.data_ptr(), xn.data_ptr(), dx.data_ptr(), B, T, Fq, Cin, Cout) == 0
            return [dx.cpu()]

        def wgrad():
            dw = torch.zeros(tasks, Cout, Cin, 3, 3).cuda()                             # the kernels accumulate onto dw
            db = torch.zeros(tasks, Cout).cuda()
            if tb:
                assert L.mtl_conv3x3_wgrad_x3_tb(st(), xn.data_ptr(), dyn.data_ptr(), am_p, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need,
                                                 B, T, Fq, Cin, Cout, tasks, dw[0].numel(), Cout) == 0
            else:
                assert L.mtl_conv3x3_wgrad_x3(st(), xn.data_ptr(), dyn.data_ptr(), am_p, dw.data_ptr(), ws.data_ptr(), need, B, T, Fq, Cin,
                                              Cout) == 0
            return [dw.cpu()]
        dx = per_task(twice(dgrad)[0])
        dw = twice(wgrad)[0]
        tag = 'pooled ' if is_pooled else ''
        for t in range(tasks):
            rep = reps[t]
            dx_ref, dw_ref = fp64_gradients(inp['x'][t], inp['w'][t], full[t])
            report(what + tag + 'data gradient task %d' % t, {'dgrad': E.rel(dx[t], dx_ref)}, rep['dgrad']['bound'], {'dgrad': rep['dgrad']['f32']})
            report(what + tag + 'weight gradient task %d' % t, {'wgrad': E.rel(dw[t], dw_ref)}, rep['wgrad']['bound'], {'wgrad': rep['wgrad']['f32']})


@pytest.mark.parametrize('shape', E.CONV_SHAPES)
def test_conv3x3_x3_keeps_all_six_terms(L, shape):
    """mtl_conv3x3_relu_fwd_x3 / _relu_pool_fwd_x3 / _dgrad_x3 (dense and pooled) / _wgrad_x3 (dense and pooled) against
    torch.nn.functional convolutions in fp64, each within B = half of the cheapest dropped term of its product in the emulation
    (on the kernel's own output: after bias + ReLU (+ pool), after the input's ReLU gate).  The backward kernels get the fp64
    reference's ReLU gates and the forward kernel's own arg-max codes, which are checked against the fp64 windows."""
    conv_case(L, shape, 1)


def test_conv3x3_x3_several_tasks_keep_all_six_terms(L):
    """the _tb entry points: three tasks with their own weights and biases in one launch, every task within its own bounds"""
    conv_case(L, E.CONV_TB[:5], E.CONV_TB[5])


@pytest.mark.parametrize('which', E.CONV_PROBES)
def test_conv3x3_x3_probe_weighs_a_second_order_term_at_2_to_the_minus_9(L, which):
    """forward: x constant-lead over a sample (positive), w antisymmetric along cin pairs, bias 0; data gradient: dy
    constant-lead, w antisymmetric along cout pairs; weight gradient: x constant-lead per channel, dy antisymmetric along
    adjacent f pairs with a zero outer ring.  Within Bp = 1/8 of the cheaper targeted drop."""
    Cin, Cout, B, T, Fq = E.CONV_PROBE_SHAPE
    inp, rep = E.conv_probe_inputs(which), E.conv_probe_report(which)
    x, w, dy = inp['x'], inp['w'], inp['dy']
    xn, dyn = dev(E.nhwc(x)), dev(E.nhwc(dy))
    w3f, w3d = wprep(L, dev(w.unsqueeze(0)), Cin, Cout)
    if which == 'fwd':
        zero = torch.zeros(Cout).cuda()

        def run():
            y = torch.full((B, T, Fq, Cout), float('nan')).cuda()
            assert L.mtl_conv3x3_relu_fwd_x3(st(), xn.data_ptr(), w3f.data_ptr(), zero.data_ptr(), y.data_ptr(), B, T, Fq, Cin, Cout) == 0
            return [E.nhwc(y.cpu())]
        want = torch.relu(F.conv2d(x.double(), w.double(), None, padding=1))
    elif which == 'dgrad':
        def run():
            dx = torch.full((B, T, Fq, Cin), float('nan')).cuda()
            assert L.mtl_conv3x3_dgrad_x3(st(), dyn.data_ptr(), None, w3d.data_ptr(), xn.data_ptr(), dx.data_ptr(), B, T, Fq, Cin, Cout) == 0
            return [E.nhwc(dx.cpu())]
        want = fp64_gradients(x, w, dy)[0]
    else:
        need = L.mtl_conv3x3_wgrad_x3_workspace(B, T, Fq, Cin, Cout, 0)
        ws = torch.empty(need // 4 + 64).cuda()

        def run():
            dw = torch.zeros(Cout, Cin, 3, 3).cuda()
            assert L.mtl_conv3x3_wgrad_x3(st(), xn.data_ptr(), dyn.data_ptr(), None, dw.data_ptr(), ws.data_ptr(), need, B, T, Fq, Cin, Cout) == 0
            return [dw.cpu()]
        want = fp64_gradients(x, w, dy)[1]
    got = twice(run)[0]
    report('conv probe ' + which, {which: E.rel(got, want)}, rep['bound'], {which: rep['f32']})


# ------------------------------------------------------------------------------------------------ x3 GEMM engine
def gemm_probe(L, M, N, K, side, ta, tb, batch):
    """op(A) op(B) of a probe pair on the bf16-split engine, `batch` items that share both operands (strides 0); worst item"""
    a, b = E.gemm_probe_inputs(M, N, K, side)
    rep = E.gemm_probe_report(M, N, K, side)
    lda, ldb = ((M if ta else K) + 3) // 4 * 4, ((K if tb else N) + 3) // 4 * 4
    A = torch.zeros((K if ta else M), lda)
    A[:, :(M if ta else K)] = a.t() if ta else a
    Bm = torch.zeros((N if tb else K), ldb)
    Bm[:, :(K if tb else N)] = b.t() if tb else b
    dA, dB = dev(A), dev(Bm)
    assert L.mtl_gemm_f32_ex_route(M, N, K, batch, 1, 0) == 2

    def run():
        C = torch.full((batch, M, N), float('nan')).cuda()
        assert L.mtl_gemm_f32_ex(st(), ta, tb, M, N, K, 1.0, dA.data_ptr(), lda, dB.data_ptr(), ldb, C.data_ptr(), N, None, None, 0, 0,
                                 batch, 1, 0, 0, 0, 0, M * N, 0, 0, 1, 0, 0, None, 0, None, 0, 0, 0) == 0
        return [C.cpu()]
    C = twice(run)[0]
    want = a.double() @ b.double()
    report('gemm probe %s x %d side %s ta=%d tb=%d' % ((M, N, K), batch, side, ta, tb), {'C': max(E.rel(C[i], want) for i in range(batch))},
           rep['bound'], {'C': rep['f32']})


@pytest.mark.parametrize('ta,tb', [(0, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize('side', ['a', 'b'])
@pytest.mark.parametrize('M,N,K', E.GEMM_PROBE_SHAPES)
def test_gemm_x3_probe_weighs_a_second_order_term_at_2_to_the_minus_9(L, x3_forced, M, N, K, side, ta, tb):
    """csrc/mtl_gemm_x3.hip (truncation split) on the two mirrored probes -- one operand constant-lead along K, the other
    antisymmetric along K -- in the three operand orientations the engine accepts: within Bp = 1/8 of the cheaper targeted drop
    of the truncation-split emulation.  One product of these shapes is 2 or 4 tiles: the 128-row tile configuration."""
    gemm_probe(L, M, N, K, side, ta, tb, 1)


@pytest.mark.parametrize('ta,tb', [(0, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize('side', ['a', 'b'])
def test_gemm_x3_probe_on_the_256_row_tiles(L, x3_forced, side, ta, tb):
    """the same probes at (100, 512, 2000) as a batch of 56 items: 224 tiles of 256 x 128, from which the engine takes its 256-row
    configuration (two row blocks per wave).  The items share both operands; every item within Bp."""
    gemm_probe(L, 100, 512, 2000, side, ta, tb, 56)
