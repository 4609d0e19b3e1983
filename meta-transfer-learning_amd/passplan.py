"""Which launches a pass issues, decided on the host from the parameter layout and the logged pointers alone: functions of plain
values, no device and no engine (tests/test_passplan.py runs them on the CPU, fall-back branches included -- the reference's module
tree never takes those).  `layout` is a ParamLayout: only layout.off(name), the offset in floats, is read.
"""
RELU, ACCUM = 1, 2      # flags of the product calls (PassEngine.gemm)

FULL = {'q': 'query', 'k': 'key', 'v': 'value'}
_LOW_RANK = ('_linear_a.weight', '_linear_b.weight', '_linear_b.bias')      # the parameters of one rank-r projection


def round_width(T, quantum):
    """Frame count rounded up to a repeating width: a multiple of `quantum`, coarser for long batches (at most 1/16 of the width, so the
    padding stays below ~6 % while a 5000-frame workload -- 55 GB of buffers per width -- sees a handful of widths, not dozens)."""
    q = max(int(quantum), 1)
    q = max(q, (T // 16) // q * q)
    return -(-T // q) * q


def pstride(layout, pre, names, suffix):
    """Distance (floats) between consecutive projections' parameters `suffix` in the flat buffer (0 for a single one)."""
    if len(names) == 1:
        return 0
    offs = [layout.off(pre + FULL[nm] + suffix) for nm in names]
    return offs[1] - offs[0]


def qkv_groups(layout, pre, xq, Mq, xkv, Mk, hk, hv):
    """[(names, input pointer, rows)]: projections that can share one strided-batch launch."""
    def uniform(names):
        for sfx in _LOW_RANK:
            offs = [layout.off(pre + FULL[nm] + sfx) for nm in names]
            steps = {b - a for a, b in zip(offs, offs[1:])}
            if len(steps) != 1 or min(steps) <= 0 or min(steps) % 4:
                return False
        return hk == hv
    if xq == xkv and Mq == Mk and uniform('qkv'):
        return [('qkv', xq, Mq)]
    if uniform('kv'):
        return [('q', xq, Mq), ('kv', xkv, Mk)]
    return [('q', xq, Mq), ('k', xkv, Mk), ('v', xkv, Mk)]


def cross_kv_plan(layout, n_dec, dk, dv):
    """(layer stride, projection stride) in floats when the K / V low-rank parameters of the decoder layers' encoder_attn blocks
    sit at constant strides in the flat buffer (they do for the reference's module tree), else None."""
    if n_dec < 2 or dk != dv:
        return None
    plan = None
    for sfx in _LOW_RANK:
        k = [layout.off('decoder.layers.%d.encoder_attn.key%s' % (i, sfx)) for i in range(n_dec)]
        v = [layout.off('decoder.layers.%d.encoder_attn.value%s' % (i, sfx)) for i in range(n_dec)]
        ls = {b - a for a, b in zip(k, k[1:])}
        ps = {b - a for a, b in zip(k, v)}
        if len(ls) != 1 or len(ps) != 1 or min(ls) <= 0 or min(ps) <= 0 or (min(ls) | min(ps)) % 4:
            return None
        if plan is not None and plan != (min(ls), min(ps)):
            return None
        plan = (min(ls), min(ps))
    return plan


def merge_wgrad_jobs(log, sG):
    """The logged weight-gradient products (PassEngine.wgrad_job: {job shape: [(C, A, B, rowsum) addresses]}) as an ordered list
    of (positional args, keyword args) for PassEngine.gemm; sG: task stride of the gradient stack.  The entries of a kind differ
    only in their four pointers; when those advance by constant strides from layer to layer (they do: per-layer buffers and the
    parameters of a stack sit at constant strides) the whole kind is ONE launch with the layer as outer batch index -- 4 x the
    workgroups of a single layer's product (64 tiles: a quarter of the chip), a quarter of the launches and no fork per sub-layer
    block.  Otherwise (a step that varies, or is no multiple of 16 bytes) one launch per entry."""
    calls = []
    for (kind, M, N, K, lda, ldb, ldc, n, sA, sB, sC, srow, has_rs), items in log.items():
        items = sorted(items)
        nl = len(items)
        steps = [tuple(b[j] - a[j] for j in range(4)) for a, b in zip(items, items[1:])]
        merged = nl > 1 and all(st == steps[0] for st in steps) and all(v % 16 == 0 for v in steps[0])
        tk = (K * lda, K * ldb, sG, 0, sG)       # task t: its K rows of dy / x, its slice of the gradient stack
        if merged:
            dC, dA, dB, dR = (v // 4 for v in steps[0])
            C0, A0, B0, R0 = items[0]
            calls.append(((1, 0, M, N, K, A0, lda, B0, ldb, C0, ldc),
                          dict(flags=ACCUM, batch=nl * n, H=n, sA=(dA, sA), sB=(dB, sB), sC=(dC, sC),
                               rowsum=R0 if has_rs else None, srow=dR, srow_h=srow, task=tk)))
        else:
            for C0, A0, B0, R0 in items:
                calls.append(((1, 0, M, N, K, A0, lda, B0, ldb, C0, ldc),
                              dict(flags=ACCUM, batch=n, sA=(sA, 0), sB=(sB, 0), sC=(sC, 0),
                                   rowsum=R0 if has_rs else None, srow=srow, task=tk)))
    return calls
