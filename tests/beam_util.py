"""Helpers of the device-ranked beam search tests: a numpy restatement of one mtl_beam_rank position, the state layout of
include/mtl_hip.h, and the decision margin of a beam search on the CPU oracle."""
import numpy as np
import torch

HDR = 4


def state_offsets(U, W, S):
    o_score = HDR * U
    o_bp = o_score + U * W
    o_tk = o_bp + U * S * W
    o_en = o_tk + U * S * W
    return o_score, o_bp, o_tk, o_en, o_en + 5 * U * S * W


def new_state(U, W, S, live, scores, done=None, ended=None):
    """state words for U utterances: live[u] rows with fp32 scores[u][:live[u]]; tables filled with -7 so that untouched words show"""
    o_score, o_bp, o_tk, o_en, n = state_offsets(U, W, S)
    st = np.full(n, -7, dtype=np.int32)
    for u in range(U):
        st[HDR * u:HDR * u + 4] = [live[u], 0 if done is None else done[u], 0 if ended is None else ended[u], 0]
        sc = np.zeros(W, dtype=np.float32)
        sc[:live[u]] = scores[u][:live[u]]
        st[o_score + u * W:o_score + (u + 1) * W] = sc.view(np.int32)
    return st


def rank_position(state, logits, lse, tok, parent, i, T4, U, W, V, S, eos):
    """what mtl_beam_rank does for position i, in numpy, IN PLACE on state / tok / parent (the selection rule of include/mtl_hip.h)"""
    o_score, o_bp, o_tk, o_en, _ = state_offsets(U, W, S)
    logits = np.asarray(logits, dtype=np.float32).reshape(U * W, V)
    lse = np.asarray(lse, dtype=np.float32)
    for u in range(U):
        hdr = state[HDR * u:HDR * u + 4]
        if hdr[1]:
            continue
        n = int(hdr[0])
        score = state[o_score + u * W:o_score + (u + 1) * W].view(np.float32)
        cands = []                                                    # (score, row, rank, token) in (row, rank) order
        for r in range(n):
            local = logits[u * W + r] - lse[u * W + r]                # fp32
            order = sorted(range(V), key=lambda v: (-local[v], v))[:W]     # largest first, lower id on equal values
            for j, v in enumerate(order):
                cands.append((np.float32(score[r] + local[v]), r, j, v))
        keep = sorted(range(len(cands)), key=lambda c: (-cands[c][0], c))[:W]      # stable: the earlier (row, rank) pair on equal scores
        force = i == T4 - 1
        ne, nl = int(hdr[2]), 0
        new_scores = []
        for c in keep:
            sc, r, _j, v = cands[c]
            if force or v == eos:
                e = o_en + 5 * (u * S * W + ne)
                state[e:e + 5] = [i, np.array([sc], dtype=np.float32).view(np.int32)[0], r, v, 1 if force else 0]
                ne += 1
            else:
                new_scores.append(sc)
                state[o_bp + (u * S + i) * W + nl] = r
                state[o_tk + (u * S + i) * W + nl] = v
                tok[u * W + nl] = v
                parent[u * W + nl] = u * W + r
                nl += 1
        score[:nl] = new_scores
        for r in range(nl, W):
            tok[u * W + r] = eos
            parent[u * W + r] = u * W if nl else u * W + r
        hdr[0], hdr[2] = nl, ne
        if nl == 0:
            hdr[1] = 1


def oracle_beam_margin(model, padded_input, input_lengths, start_token, beam_width, tgt_max_len, eos_id=2):
    """Smallest decision margin of the beam search of oracle.refimpl.beam_search on this batch: over all utterances and positions, the gap
    between the W-th and the (W + 1)-th best candidate score (candidates: every live hypothesis' expansions).  CPU, oracle model."""
    import torch.nn.functional as F
    W = int(beam_width)
    model.eval()
    margin = float('inf')
    with torch.no_grad():
        f = model.conv(padded_input)
        B, C, H, Wd = f.shape
        mem_all = model.encoder(f.view(B, C * H, Wd).transpose(1, 2).contiguous(), input_lengths)
        dec = model.decoder
        max_len = mem_all.shape[1]
        for b in range(B):
            mem = mem_all[b:b + 1]
            hyps = [dict(score=0.0, yseq=torch.full((1, 1), int(start_token), dtype=torch.int64))]
            for i in range(tgt_max_len):
                cands = []
                for hyp in hyps:
                    ys = hyp['yseq']
                    Lq = ys.shape[1]
                    future = torch.triu(torch.ones(Lq, Lq, dtype=torch.bool), diagonal=1).unsqueeze(0)
                    x = dec.trg_embedding(ys) + dec.positional_encoding.pe[:, :Lq]
                    for layer in dec.layers:
                        x = layer(x, mem, torch.ones(1, Lq, 1), future, torch.zeros(1, Lq, max_len, dtype=torch.bool))
                    local = F.log_softmax(dec.output_linear(x[:, -1]), dim=1)
                    best, ids = torch.topk(local, W + 1, dim=1)
                    for j in range(W + 1):
                        cands.append(dict(score=hyp['score'] + best[0, j], yseq=torch.cat([ys, ids[0, j].view(1, 1)], dim=1)))
                cands = sorted(cands, key=lambda h: h['score'], reverse=True)
                margin = min(margin, float(cands[W - 1]['score'] - cands[W]['score']))
                hyps = [h for h in cands[:W] if int(h['yseq'][0, -1]) != eos_id]
                if i == max_len - 1 or not hyps:
                    break
    model.train()
    return margin


def oracle_greedy_margin(model, padded_input, input_lengths, start_token, steps):
    """Smallest decision margin of oracle.refimpl.greedy_search on this batch: over all rows and steps, the gap between the best and the
    second-best log-probability of the step.  Not oracle_beam_margin with W = 1: the greedy search does not stop at EOS and takes exactly
    `steps` steps for every row (and the whole batch goes through the decoder at once, as greedy_search does).  CPU, oracle model."""
    import torch.nn.functional as F
    model.eval()
    margin = float('inf')
    with torch.no_grad():
        f = model.conv(padded_input)
        B, C, H, Wd = f.shape
        mem = model.encoder(f.view(B, C * H, Wd).transpose(1, 2).contiguous(), input_lengths)
        dec = model.decoder
        ys = torch.full((B, 1), int(start_token), dtype=torch.int64)
        for _ in range(steps):
            Lq = ys.shape[1]
            future = torch.triu(torch.ones(Lq, Lq, dtype=torch.bool), diagonal=1).unsqueeze(0).expand(B, Lq, Lq)
            x = dec.trg_embedding(ys) + dec.positional_encoding.pe[:, :Lq]
            for layer in dec.layers:
                x = layer(x, mem, torch.ones(B, Lq, 1), future, torch.zeros(B, Lq, mem.shape[1], dtype=torch.bool))
            best, ids = torch.topk(F.log_softmax(dec.output_linear(x)[:, -1], dim=1), 2, dim=1)
            margin = min(margin, float((best[:, 0] - best[:, 1]).min()))
            ys = torch.cat([ys, ids[:, :1]], dim=1)
    model.train()
    return margin
