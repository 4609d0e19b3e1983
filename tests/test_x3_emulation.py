"""CPU: every bound of tests/test_x3_precision_gpu.py separates the six-term split-bf16 product from any five-term one.

For every case of the GPU file, on the same inputs (tests/x3_emul.py builds them for both files):
* random inputs: the bound B is half of what the cheapest dropped second-order term costs against fp64 (largest relative-L2 error
  over the outputs); the case is admitted only if the six-term emulation stays within B / 3 and torch fp32 within B / 2 on every
  output;
* probes (the leading piece product cancels, a second-order term weighs 2^-9 of the result): Bp is an eighth of the cheaper of the
  two targeted drops; admitted only if the six-term emulation stays within Bp / 4;
* every five-term emulation, handed to the assertion helper the GPU tests use, fails it.
Run with -s to see B / Bp per case."""
import pytest
import torch

from tests import x3_emul as E

ATTN = sorted(E.ATTN_CASES)
ATTN_PROBES = sorted(E.ATTN_PROBES)
CONV = [(s, 1, pooled, 0) for s in E.CONV_SHAPES for pooled in (False, True)]
CONV += [(E.CONV_TB[:5], E.CONV_TB[5], pooled, task) for pooled in (False, True) for task in range(E.CONV_TB[5])]      # every task of the _tb case
GEMM_PROBES = [(M, N, K, side) for (M, N, K) in E.GEMM_PROBE_SHAPES for side in 'ab']


def _say(what, r, six, f32):
    print('\n%-44s bound %.3e   six terms %.3e (bound / %.1f)   torch fp32 %.3e (bound / %.1f)   cheapest drop %.3e' % (
        what, r['bound'], six, r['bound'] / six, f32, r['bound'] / f32,
        min(max(e[o] for o in r['outputs']) if isinstance(e, dict) else e for e in r['drops'].values())))


@pytest.mark.parametrize('rounding', ['rne', 'trunc'])
def test_split3_is_exact(rounding):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4096, generator=g)
    for t in (x, x * 2.0 ** 60, x * 2.0 ** -60, torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, 1.0 + 2.0 ** -23])):
        p = E.split3(t, rounding)                               # asserts p0 + p1 + p2 == x
        for piece in p:
            assert torch.equal(piece, piece.bfloat16().float())             # every piece is a bf16 value
    z = E.split3(torch.tensor([0.0, -0.0]), rounding)
    assert all(float(p.abs().max()) == 0.0 for p in z)
    a, b = torch.randn(5, 8, generator=g), torch.randn(8, 3, generator=g)
    nine = tuple((i, j) for i in range(3) for j in range(3))
    assert E.rel(E.mm_x3(a, b, nine, rounding), a.double() @ b.double()) < 3e-7            # all nine terms: the exact product
    assert len(E.drops()) == 3 and all(len(d) == 5 and (0, 0) in d and (1, 0) in d and (0, 1) in d for d in E.drops())


def test_probe_builders_cancel_the_leading_term():
    g = torch.Generator().manual_seed(8)
    for rounding in ('rne', 'trunc'):
        a, b = E.const_lead((37, 64), g=g, rounding=rounding), E.antisym((29, 64), g=g).t()
        pa, pb = E.split3(a, rounding), E.split3(b.contiguous(), rounding)
        for j in range(3):          # a0 . b_j vanishes in exact arithmetic: every piece of an antisymmetric operand is antisymmetric
            assert float((pa[0].double() @ pb[j].double()).abs().max()) == 0.0
        lead = (pa[1].double() @ pb[0].double()).norm()
        for t in ((1, 1), (2, 0)):  # ... and the two probed terms weigh about 2^-9 of the carrying one, not 2^-18
            assert float((pa[t[0]].double() @ pb[t[1]].double()).norm() / lead) > 2.0 ** -11


def test_attention_memo_only_saves_time():
    """the sweep over drops reuses piece products of the six-term run; with or without that, every output is bit-identical"""
    inp = E.attn_inputs('one_full_tile')
    args, kw = E._attn_args(inp)
    memo = {}
    E.attention_x3(*args, memo=memo, **kw)
    for drop in (('qk', (1, 1)), ('pv', (2, 0)), ('dov', (0, 2)), ('dsq', (1, 1))):
        a, b = E.attention_x3(*args, drop=drop, memo=memo, **kw), E.attention_x3(*args, drop=drop, **kw)
        assert all(torch.equal(a[n], b[n]) for n in a), drop


@pytest.mark.parametrize('name', ATTN)
def test_attention_case_is_admitted(name):
    r = E.attn_report(name)
    six, f32 = (max(r[k][o] for o in E.ATTN_OUTPUTS) for k in ('six', 'f32'))
    _say('attention ' + name, r, six, f32)
    assert len(r['drops']) == 18
    E.check({o: r['six'][o] for o in E.ATTN_OUTPUTS}, r['bound'] / 3, 'six terms')
    E.check({o: r['f32'][o] for o in E.ATTN_OUTPUTS}, r['bound'] / 2, 'torch fp32')
    E.check({'lse': r['six']['lse']}, r['bound'] / 3, 'six terms')
    assert 5e-7 < r['bound'] < 2e-6                             # fp32-class: the bound is not met by losing 2^-18 of a product


@pytest.mark.parametrize('name', ATTN_PROBES)
def test_attention_probe_is_admitted(name):
    r = E.attn_report(name)
    six, f32 = (max(r[k][o] for o in r['outputs']) for k in ('six', 'f32'))
    _say('attention probe ' + name, r, six, f32)
    assert len(r['drops']) == 2
    E.check({o: r['six'][o] for o in r['outputs']}, r['bound'] / 4, 'six terms')
    for e in r['drops'].values():
        assert max(e[o] for o in r['outputs']) >= 8 * r['bound']


@pytest.mark.parametrize('shape,tasks,pooled,task', CONV)
def test_convolution_case_is_admitted(shape, tasks, pooled, task):
    rep = E.conv_report(shape, tasks, pooled, task)
    for n in E.CONV_PRODUCTS:
        r = rep[n]
        _say('conv %s task %d of %d pooled=%d %s' % (shape, task, tasks, pooled, n), r, r['six'], r['f32'])
        assert len(r['drops']) == 3
        E.check({n: r['six']}, r['bound'] / 3, 'six terms')
        E.check({n: r['f32']}, r['bound'] / 2, 'torch fp32')
        assert 5e-7 < r['bound'] < 2e-6


@pytest.mark.parametrize('which', E.CONV_PROBES)
def test_convolution_probe_is_admitted(which):
    r = E.conv_probe_report(which)
    _say('conv probe ' + which, r, r['six'], r['f32'])
    assert len(r['drops']) == 2 and min(r['drops'].values()) >= 8 * r['bound']
    E.check({which: r['six']}, r['bound'] / 4, 'six terms')


@pytest.mark.parametrize('M,N,K,side', GEMM_PROBES)
def test_gemm_probe_is_admitted(M, N, K, side):
    r = E.gemm_probe_report(M, N, K, side)
    _say('gemm probe %s %s' % ((M, N, K), side), r, r['six'], r['f32'])
    assert len(r['drops']) == 2 and min(r['drops'].values()) >= 8 * r['bound']
    E.check({'C': r['six']}, r['bound'] / 4, 'six terms')


@pytest.mark.parametrize('M,N,K', E.GEMM_RECORD_SHAPES)
def test_truncation_split_makes_the_gemm_engines_bound_sensitive(M, N, K):
    """regression record: the x3 GEMM engine splits by truncation, whose second pieces are twice as large as rounded ones -- a
    dropped term costs >= 4 x the 2e-6 of test_bf16_split_engine_contract and six terms stay <= 1/4 of it, so that test needs no
    tighter random-input bound"""
    r = E.gemm_record_report(M, N, K)
    _say('gemm (truncation) %s' % ((M, N, K),), r, r['six'], r['f32'])
    assert min(r['drops'].values()) >= 4 * E.GEMM_BOUND_FP32_TEST
    assert r['six'] <= E.GEMM_BOUND_FP32_TEST / 4


def _mutants():
    out = [('attn', n, m) for n in ATTN for m in [(p, t) for p in E.ATTN_PRODUCTS for t in E.SECOND_ORDER]]
    out += [('attn', n, (E.ATTN_PROBES[n][0], t)) for n in ATTN_PROBES for t in E.PROBE_TERMS[E.ATTN_PROBES[n][1]]]
    out += [('conv', c, (n, t)) for c in CONV for n in E.CONV_PRODUCTS for t in E.SECOND_ORDER]
    out += [('convprobe', w, (w, t)) for w in E.CONV_PROBES for t in E.PROBE_TERMS[E.CONV_PROBE_SIDE[w]]]
    out += [('gemm', c, ('C', t)) for c in GEMM_PROBES for t in E.PROBE_TERMS[c[3]]]
    return out


@pytest.mark.parametrize('kind,case,mutant', _mutants())
def test_every_five_term_product_fails_the_gpu_assertion(kind, case, mutant):
    """sensitivity without touching a kernel: the emulation with one second-order term removed from one product goes through
    the assertion of the GPU tests (x3_emul.check with the case's bound) and must fail it"""
    if kind == 'attn':
        r = E.attn_report(case)
        errs = {o: r['drops'][mutant][o] for o in r['outputs']}
    elif kind == 'conv':
        r = E.conv_report(*case)[mutant[0]]
        errs = {mutant[0]: r['drops'][mutant[1]]}
    else:
        r = E.conv_probe_report(case) if kind == 'convprobe' else E.gemm_probe_report(*case)
        errs = {mutant[0]: r['drops'][mutant[1]]}
    with pytest.raises(AssertionError):
        E.check(errs, r['bound'], 'five terms')
