"""passplan on the CPU: the host decisions about which launches a pass issues, with the fall-back branches the reference's module tree
never takes (parameter strides that vary, steps that are no multiple of 16 bytes, a single decoder layer, h d_k != h d_v).  The figures
are those PassEngine's own methods gave on the same inputs before they became functions."""
import pytest

D, R, HK = 32, 8, 16
SUFFIXES = ('_linear_a.weight', '_linear_b.weight', '_linear_b.bias')


@pytest.fixture(scope='module')
def pp():
    import mtl_amd  # noqa: F401
    from mtl_amd import passplan
    return passplan


def _block(pre, order=('query', 'key', 'value'), hv=HK):
    """one attention block's low-rank projections: 256 + 128 + 16 = 400 floats each at hk = hv = 16"""
    out = []
    for proj in order:
        w = hv if proj == 'value' else HK
        out += [(pre + proj + SUFFIXES[0], (R, D)), (pre + proj + SUFFIXES[1], (w, R)), (pre + proj + SUFFIXES[2], (w,))]
    return out


def _layout(named_shapes):
    from mtl_amd.engine import ParamLayout
    return ParamLayout(named_shapes)


def _cross(n, extra_before=None):
    shapes = []
    for i in range(n):
        if i == extra_before:
            shapes.append(('decoder.layers.%d.extra' % i, (12,)))
        shapes += _block('decoder.layers.%d.encoder_attn.' % i)
    return _layout(shapes)


def test_cross_kv_plan_needs_constant_strides_two_layers_and_equal_head_sizes(pp):
    assert pp.cross_kv_plan(_cross(3), 3, 16, 16) == (1200, 400)
    assert pp.cross_kv_plan(_cross(2), 2, 16, 16) == (1200, 400)
    assert pp.cross_kv_plan(_cross(3), 1, 16, 16) is None
    assert pp.cross_kv_plan(_cross(3), 3, 16, 32) is None
    assert pp.cross_kv_plan(_cross(3, extra_before=2), 3, 16, 16) is None            # layer steps 1200, then 1212
    assert pp.cross_kv_plan(_cross(3, extra_before=0), 3, 16, 16) == (1200, 400)     # (in front of all layers: no step changes)


def test_qkv_groups_share_a_launch_only_over_one_input_and_uniform_parameters(pp):
    pre = 'decoder.layers.0.self_attn.'
    L = _layout(_block(pre))
    names = lambda groups: [g[0] for g in groups]
    assert pp.qkv_groups(L, pre, 1000, 6, 1000, 6, HK, HK) == [('qkv', 1000, 6)]
    assert pp.qkv_groups(L, pre, 1000, 6, 2000, 6, HK, HK) == [('q', 1000, 6), ('kv', 2000, 6)]
    assert pp.qkv_groups(L, pre, 1000, 6, 1000, 9, HK, HK) == [('q', 1000, 6), ('kv', 1000, 9)]
    assert pp.qkv_groups(_layout(_block(pre, hv=32)), pre, 1000, 6, 1000, 6, 16, 32) == [('q', 1000, 6), ('k', 1000, 6), ('v', 1000, 6)]
    swapped = _layout(_block(pre, order=('query', 'value', 'key')))                   # key behind value: a negative stride
    assert names(pp.qkv_groups(swapped, pre, 1000, 6, 1000, 6, HK, HK)) == ['q', 'k', 'v']
    assert names(pp.qkv_groups(swapped, pre, 1000, 6, 2000, 6, HK, HK)) == ['q', 'k', 'v']


def test_pstride_is_the_distance_of_the_first_two_projections(pp):
    pre = 'decoder.layers.0.self_attn.'
    L = _layout(_block(pre))
    for sfx in SUFFIXES:
        assert pp.pstride(L, pre, 'q', sfx) == 0 and pp.pstride(L, pre, 'v', sfx) == 0
        assert pp.pstride(L, pre, 'qkv', sfx) == 400 and pp.pstride(L, pre, 'kv', sfx) == 400
    swapped = _layout(_block(pre, order=('query', 'value', 'key')))
    assert pp.pstride(swapped, pre, 'kv', SUFFIXES[0]) == -400 and pp.pstride(swapped, pre, 'qkv', SUFFIXES[0]) == 800


def test_round_width_is_the_one_function(pp):
    from mtl_amd import engine
    assert engine.round_width is pp.round_width
    assert [pp.round_width(T, 64) for T in (1, 64, 65, 1000, 5000)] == [64, 64, 128, 1024, 5120]
    assert pp.round_width(7, 0) == 7


SG, M, N, K, LDA, LDB, LDC = 1000, 8, 4, 6, 8, 4, 4
HEAD = (1, 0, M, N, K)


def _key(kind='e*.ff.w1', n=1, sA=0, sB=0, sC=0, srow=0, has_rs=True):
    return (kind, M, N, K, LDA, LDB, LDC, n, sA, sB, sC, srow, has_rs)


def _ptrs(l, c_step=160, rowsum=True):
    return (100000 + c_step * l, 4096 + 64 * l, 8192 + 32 * l, 200000 + 48 * l if rowsum else 0)


def test_layers_at_constant_steps_merge_into_one_launch(pp):
    log = {_key(): [_ptrs(2), _ptrs(0), _ptrs(1)]}
    assert pp.merge_wgrad_jobs(log, SG) == [
        (HEAD + (4096, 8, 8192, 4, 100000, 4),
         dict(flags=pp.ACCUM, batch=3, H=1, sA=(16, 0), sB=(8, 0), sC=(40, 0), rowsum=200000, srow=12, srow_h=0,
              task=(48, 24, 1000, 0, 1000)))]
    # inner items of a job (n, sA, sB, sC, srow) become the inner batch index of the merged launch
    (a, kw), = pp.merge_wgrad_jobs({_key(n=2, sA=7, sB=9, sC=11, srow=5): [_ptrs(1), _ptrs(0)]}, SG)
    assert a == HEAD + (4096, 8, 8192, 4, 100000, 4)
    assert kw == dict(flags=pp.ACCUM, batch=4, H=2, sA=(16, 7), sB=(8, 9), sC=(40, 11), rowsum=200000, srow=12, srow_h=5,
                      task=(48, 24, 1000, 0, 1000))


def test_steps_that_vary_or_are_not_16_byte_multiples_fall_back_to_single_launches(pp):
    single = lambda C, A, B: (HEAD + (A, 8, B, 4, C, 4),
                              dict(flags=pp.ACCUM, batch=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), rowsum=None, srow=0, task=(48, 24, 1000, 0, 1000)))
    # C steps of 160, then 176
    items = [(100000 + 336, 4096 + 128, 8192 + 64, 0), _ptrs(0, rowsum=False), _ptrs(1, rowsum=False)]
    assert pp.merge_wgrad_jobs({_key(has_rs=False): items}, SG) == [
        single(100000, 4096, 8192), single(100160, 4160, 8224), single(100336, 4224, 8256)]
    # a step of 8 bytes
    assert pp.merge_wgrad_jobs({_key(has_rs=False): [_ptrs(1, c_step=8, rowsum=False), _ptrs(0, c_step=8, rowsum=False)]}, SG) == [
        single(100000, 4096, 8192), single(100008, 4160, 8224)]
    # one job: its own inner batch
    (a, kw), = pp.merge_wgrad_jobs({_key(n=3, sA=7, sB=9, sC=11, srow=5): [_ptrs(0)]}, SG)
    assert a == HEAD + (4096, 8, 8192, 4, 100000, 4)
    assert kw == dict(flags=pp.ACCUM, batch=3, sA=(7, 0), sB=(9, 0), sC=(11, 0), rowsum=200000, srow=5, task=(48, 24, 1000, 0, 1000))


def test_kinds_keep_their_order_and_the_log_is_left_as_it_was(pp):
    first, second = [_ptrs(1), _ptrs(0)], [_ptrs(0, rowsum=False)]
    log = {_key('d*.sa.ob'): first, _key('e*.ff.w1', has_rs=False): second}
    calls = pp.merge_wgrad_jobs(log, 0)
    assert [kw['batch'] for _, kw in calls] == [2, 1] and [kw['rowsum'] for _, kw in calls] == [200000, None]
    assert all(kw['task'] == (48, 24, 0, 0, 0) for _, kw in calls)
    assert first == [_ptrs(1), _ptrs(0)]
