"""fp64 restatement of the CTC loss the device computes (mtl_ctc_fwd / mtl_ctc_bwd, include/mtl_hip.h) and the case table the CPU
and GPU tests share.

Semantics (utils/metrics.py:127-148 of the reference = F.ctc_loss(log_softmax(pred), gold, sizes, trg_lengths, 'mean')):
  nll[u]   -log p(labels_u | rows 0..in_len[u]-1): +inf when no alignment exists (reduction='none', zero_infinity=False);
           in_len = 0 gives 0 for an empty target and +inf otherwise; a label outside [0, V) makes the utterance infeasible
  loss[g]  mean over the per_group utterances of group g of nll_u / max(tgt_len_u, 1)            (per_group = U: reduction='mean')
  dlogits  gscale [* gscale_dev[g]] / (per_group max(tgt_len_u, 1)) * (softmax - label posterior) on rows t < in_len[u] of a feasible
           utterance, exactly 0 on the other rows and on every row of an infeasible utterance (torch's zero_infinity=True gradient)
The extended label sequence is blank, l1, blank, l2, ..., blank; the skip s-2 -> s is allowed where the two labels differ (compared by
value, as torch does: a label equal to the blank is an ordinary label that shares the blank's column)."""
import numpy as np

NEG = -np.inf


def in_len_from_percentages(pct, Td):
    """sizes = src_percentages.mul_(Td).int(): an fp32 product, truncated"""
    return (np.asarray(pct, dtype=np.float32) * np.float32(Td)).astype(np.int32)


def _lse_rows(*rows):
    """log(sum(exp(rows))) elementwise; -inf where every operand is -inf"""
    m = rows[0]
    for r in rows[1:]:
        m = np.maximum(m, r)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = sum(np.exp(np.where(m == NEG, NEG, r - np.where(m == NEG, 0.0, m))) for r in rows)
        return np.where(m == NEG, NEG, m + np.log(s))


def _shift(a, k, rev=False):
    out = np.full_like(a, NEG)
    if k < a.shape[0]:
        if rev:
            out[:a.shape[0] - k] = a[k:]
        else:
            out[k:] = a[:a.shape[0] - k]
    return out


def utterance(logits, labels, Tin, blank=0):
    """logits (T, V) float64, labels (L,) ints, Tin rows used -> (nll, d nll / d logits (T, V) with zero rows beyond Tin, or all zero
    when nll = +inf)"""
    T, V = logits.shape
    labels = np.asarray(labels, dtype=np.int64)
    L = labels.shape[0]
    grad = np.zeros((T, V))
    if L and (labels.min() < 0 or labels.max() >= V):
        return np.inf, grad
    if Tin == 0:
        return (0.0 if L == 0 else np.inf), grad
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, dtype=bool)
    skip[2:] = ext[2:] != ext[:-2]
    x = logits[:Tin]
    mx = x.max(1, keepdims=True)
    lp = x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))
    lpe = lp[:, ext]                                              # (Tin, S)
    alpha = np.full((Tin, S), NEG)
    alpha[0, :2] = lpe[0, :2]
    for t in range(1, Tin):
        a = alpha[t - 1]
        r = _lse_rows(a, _shift(a, 1), np.where(skip, _shift(a, 2), NEG))
        alpha[t] = np.where(r == NEG, NEG, r + lpe[t])
    ll = _lse_rows(alpha[-1, S - 1:S], alpha[-1, S - 2:S - 1] if S > 1 else np.full(1, NEG))[0]
    if ll == NEG:
        return np.inf, grad
    beta = np.full((Tin, S), NEG)
    beta[-1, max(S - 2, 0):] = lpe[-1, max(S - 2, 0):]
    skip_fwd = np.zeros(S, dtype=bool)
    skip_fwd[:-2] = skip[2:]
    for t in range(Tin - 2, -1, -1):
        b = beta[t + 1]
        r = _lse_rows(b, _shift(b, 1, True), np.where(skip_fwd, _shift(b, 2, True), NEG))
        beta[t] = np.where(r == NEG, NEG, r + lpe[t])
    reach = (alpha != NEG) & (beta != NEG)
    with np.errstate(invalid='ignore'):
        post = np.where(reach, np.exp(np.where(reach, alpha + beta - lpe - ll, 0.0)), 0.0)
    grad[:Tin] = np.exp(lp)
    np.subtract.at(grad, (np.repeat(np.arange(Tin), S), np.tile(ext, Tin)), post.reshape(-1))
    return -ll, grad


def ctc(logits, gold, in_len, tgt_len, blank=0, per_group=None, gscale=1.0, gscale_dev=None):
    """logits (U, T, V), gold (U, ldg), in_len / tgt_len (U) -> nll (U), loss (U / per_group), dlogits (U, T, V); all float64.
    The lengths are clamped like the kernels clamp them: in_len to [0, T], tgt_len to [0, ldg]."""
    logits = np.asarray(logits, dtype=np.float64)
    U, T, V = logits.shape
    gold = np.asarray(gold)
    per_group = U if per_group is None else per_group
    nll = np.zeros(U)
    grad = np.zeros((U, T, V))
    Ls = np.clip(np.asarray(tgt_len, dtype=np.int64), 0, gold.shape[1])
    Ts = np.clip(np.asarray(in_len, dtype=np.int64), 0, T)
    for u in range(U):
        nll[u], g = utterance(logits[u], gold[u, :Ls[u]], int(Ts[u]), blank)
        s = gscale * (1.0 if gscale_dev is None else float(gscale_dev[u // per_group])) / (per_group * max(int(Ls[u]), 1))
        grad[u] = s * g
    with np.errstate(invalid='ignore'):
        loss = (nll / np.maximum(Ls, 1)).reshape(-1, per_group).sum(1) / per_group
    return nll, loss, grad


def feasible(labels, Tin):
    """an alignment exists iff the rows cover the labels plus one blank between adjacent equal labels"""
    labels = list(labels)
    return Tin >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:])) and (Tin > 0 or not labels)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table: the smallest shapes at which the kernels take another path
# ---------------------------------------------------------------------------------------------------------------------------------
def _no_adjacent_repeats(rng, n, V):
    out = []
    for _ in range(n):
        c = int(rng.integers(1, V))
        while out and c == out[-1]:
            c = int(rng.integers(1, V))
        out.append(c)
    return out


def _case(name, V, T, targets, in_len, scale, seed, per_group=None, ldg=None):
    rng = np.random.default_rng(seed)
    U = len(targets)
    ldg = max(max((len(t) for t in targets), default=0) + 1, 1) if ldg is None else ldg
    gold = np.zeros((U, ldg), dtype=np.int64)
    for u, t in enumerate(targets):
        gold[u, :len(t)] = t
    logits = (rng.standard_normal((U, T, V)) * scale).astype(np.float32)
    return dict(name='%s-x%d' % (name, scale), V=V, T=T, U=U, gold=gold, in_len=np.asarray(in_len, dtype=np.int32),
                tgt_len=np.asarray([len(t) for t in targets], dtype=np.int32), logits=logits, per_group=U if per_group is None else per_group)


def cases():
    out = []
    for scale in (1, 12):
        rng = np.random.default_rng(100 + scale)
        # lattice widths S = 1, 3, 63, 65, 127, 129: around the wave and half the workgroup
        tg = [_no_adjacent_repeats(rng, L, 97) for L in (0, 1, 31, 32, 63, 64)]
        out.append(_case('widths', 97, 66, tg, [66, 40, 66, 50, 66, 66], scale, 1))
        # wider than any workgroup: S = 601 over 256 lanes (random labels of 6 symbols: every chain is long, many repeats)
        out.append(_case('wide', 7, 620, [[int(v) for v in rng.integers(1, 7, 300)]], [620], scale, 2))
        # one row; rows beyond in_len; no rows at all, with and without labels
        # (seed: no row whose blank holds all of the softmax -- an nll of 1e-9 is the cancellation lse - x, nothing to compare at 1e-12)
        out.append(_case('T1', 7, 1, [[], [3], [], [2]], [1, 1, 0, 0], scale, 13))
        out.append(_case('short', 7, 5, [[], [1], [2, 4], [5, 5], [6]], [0, 0, 3, 4, 5], scale, 4))
        # one repeated label (no skip transition anywhere); a target with repeats at exactly L + repeats rows (one path), one row
        # fewer (none), and with rows to spare: feasible and infeasible utterances side by side
        rep = [3, 3, 5, 5, 2]
        out.append(_case('repeats', 7, 12, [[4] * 5, [4] * 5, [4] * 5, rep, rep, rep], [12, 9, 8, 7, 6, 12], scale, 5))
        # wide vocabulary (the north-star width, a multiple of 4) and one that is not a multiple of 4 or 64
        out.append(_case('V3764', 3764, 10, [_no_adjacent_repeats(rng, 4, 3764), _no_adjacent_repeats(rng, 6, 3764)], [10, 8], scale, 6))
        # task groups
        tg = [_no_adjacent_repeats(rng, L, 97) for L in (3, 5, 2, 7, 4, 6)]
        for pg in (6, 3, 1):
            out.append(_case('groups%d' % pg, 97, 9, tg, [9, 9, 4, 9, 3, 8], scale, 8, per_group=pg))
    return out


def blank_label_cases():
    """A label equal to the blank (outside torch's contract: its value agrees, its gradient overwrites the blank column of the last
    row): here an ordinary label whose posterior joins the blank states' in the blank's column.  Checked against finite differences
    on the CPU and against this oracle on the device."""
    return [_case('blanklabel', 7, 9, [[2, 0, 0, 3], [0], [1, 0, 1]], [9, 4, 9], scale, 7) for scale in (1, 12)]
