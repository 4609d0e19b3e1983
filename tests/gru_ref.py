"""Test helper (NOT product code): torch-CPU restatement of the reference's `RNNModel` for `--model GRU` and `--tied`
(lm/model/rnn_model.py: Embedding -> dropout -> nn.GRU / nn.LSTM -> dropout -> Linear, `decoder.weight` optionally the very
`encoder.weight` Parameter), evaluated step by step from the module's own parameters so that the dropout realisations of the device
can be replayed (`masks`).  Written from the cell algebra below, runnable in fp64 (`.double()`); pinned to the real reference by
tests/golden/LG0.npz (tests/test_lm_gru.py).

GRU cell, torch gate order r | z | n, with gx = x W_ih^T + b_ih and gh = h W_hh^T + b_hh:
    r = sigmoid(gx_r + gh_r)   z = sigmoid(gx_z + gh_z)   q = gh_n   n = tanh(gx_n + r q)   h' = (1 - z) n + z h
backward for dh' (gradient from above + recurrent gradient + direct carry):
    dn = dh' (1 - z)   dz = dh' (h - n)   carry = dh' z   da_n = dn (1 - n^2)   dq = da_n r   da_r = da_n q r (1 - r)   da_z = dz z (1 - z)
    dgx = [da_r, da_z, da_n]   dgh = [da_r, da_z, dq]
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def gru_cell(gx, gh, h):
    """gx, gh (B, 3H), h (B, H) -> (h', acts (B, 4H) = r | z | n | q)"""
    xr, xz, xn = gx.chunk(3, dim=1)
    hr, hz, q = gh.chunk(3, dim=1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * q)
    return (1 - z) * n + z * h, torch.cat([r, z, n, q], dim=1)


def gru_cell_backward(dh, acts, h_prev):
    """the hand-written formulas of the module docstring: dh (B, H) total gradient of h', acts (B, 4H), h_prev (B, H)
    -> (dgx (B, 3H), dgh (B, 3H), carry (B, H))"""
    r, z, n, q = acts.chunk(4, dim=1)
    dn, dz = dh * (1 - z), dh * (h_prev - n)
    da_n = dn * (1 - n * n)
    dq, da_r, da_z = da_n * r, da_n * q * r * (1 - r), dz * z * (1 - z)
    return torch.cat([da_r, da_z, da_n], dim=1), torch.cat([da_r, da_z, dq], dim=1), dh * z


class RNNModel(nn.Module):
    def __init__(self, rnn_type, ntoken, ninp, nhid, nlayers, dropout=0.5, tie_weights=False):
        super().__init__()
        assert rnn_type in ('LSTM', 'GRU')
        self.encoder = nn.Embedding(ntoken, ninp)
        self.rnn = getattr(nn, rnn_type)(ninp, nhid, nlayers, dropout=dropout)
        self.decoder = nn.Linear(nhid, ntoken)
        if tie_weights:
            if nhid != ninp:
                raise ValueError('When using the tied flag, nhid must be equal to emsize')
            self.decoder.weight = self.encoder.weight
        self.rnn_type, self.ntoken, self.nhid, self.nlayers = rnn_type, ntoken, nhid, nlayers
        self.encoder.weight.data.uniform_(-0.1, 0.1)
        self.decoder.bias.data.fill_(0)
        self.decoder.weight.data.uniform_(-0.1, 0.1)

    def init_hidden(self, bsz):
        z = lambda: torch.zeros(self.nlayers, bsz, self.nhid, dtype=self.decoder.bias.dtype)
        return (z(), z()) if self.rnn_type == 'LSTM' else z()

    def features(self, inp, hidden, masks=None):
        """inp (T, B) int64; hidden: (h, c) for the LSTM, h for the GRU, each (nlayers, B, nhid).  masks: None or {'emb': (T, B, ninp),
        'l0': (T, B, nhid), ..., 'out': (T, B, nhid)}: multiplicative keep-masks already scaled by 1 / (1 - p) (the recurrent module
        drops the output of every layer but the last; the model drops the embedding and the last layer's output).
        -> (top layer's dropped output (T, B, nhid), new hidden)"""
        T, B = inp.shape
        x = self.encoder(inp)
        if masks is not None:
            x = x * masks['emb'].to(x.dtype)
        lstm = self.rnn_type == 'LSTM'
        h0, c0 = hidden if lstm else (hidden, None)
        hn, cn = [], []
        for l in range(self.nlayers):
            w_ih, w_hh = getattr(self.rnn, 'weight_ih_l%d' % l), getattr(self.rnn, 'weight_hh_l%d' % l)
            b_ih, b_hh = getattr(self.rnn, 'bias_ih_l%d' % l), getattr(self.rnn, 'bias_hh_l%d' % l)
            h, c = h0[l], (c0[l] if lstm else None)
            outs = []
            for t in range(T):
                gx, gh = x[t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
                if lstm:
                    i, f, g, o = (gx + gh).chunk(4, dim=1)
                    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                    h = torch.sigmoid(o) * torch.tanh(c)
                else:
                    h, _ = gru_cell(gx, gh, h)
                outs.append(h)
            x = torch.stack(outs)
            hn.append(h)
            cn.append(c)
            if masks is not None:
                x = x * masks['l%d' % l if l < self.nlayers - 1 else 'out'].to(x.dtype)
        return x, ((torch.stack(hn), torch.stack(cn)) if lstm else torch.stack(hn))

    def forward(self, inp, hidden, masks=None):
        """-> (logits (T, B, ntoken), new hidden)"""
        T, B = inp.shape
        x, hidden = self.features(inp, hidden, masks)
        return self.decoder(x.view(T * B, self.nhid)).view(T, B, -1), hidden

    def sequence_nll(self, ids, targets):
        """summed next-word NLL per sequence of a ragged batch: ids, targets (T, B), targets -1 after a sequence's end; eval mode,
        zero initial state -> (B,)"""
        T, B = ids.shape
        out, _ = self.forward(ids, self.init_hidden(B))
        nll = F.cross_entropy(out.view(T * B, -1), targets.reshape(-1), ignore_index=-1, reduction='none')
        return nll.view(T, B).sum(0)


def detach(hidden):
    return hidden.detach() if torch.is_tensor(hidden) else tuple(h.detach() for h in hidden)


def task_weights(n, ratio):
    return [ratio if i == n - 1 else (1.0 - ratio) / max(n - 1, 1) for i in range(n)]


def clip_(grads, max_norm):
    total = torch.sqrt(sum((g.detach() ** 2).sum() for g in grads))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    for g in grads:
        g.mul_(coef)


def meta_step(model, hidden, task_batches, val_batch, lr, meta_lr_factor=3.0, clip=0.25, ratio=0.8):
    """One iteration of the first-order meta step the product's LMMetaTrainer documents (the sequence of
    oracle.lm_refimpl.meta_step, for either hidden-state form): per task a train pass at theta0 from the carried (detached) state,
    clipped inner SGD step lr / meta_lr_factor, validation pass at theta' from the state the train pass returned, G += w_i grad;
    theta0 restored; then G clipped and theta <- theta0 - lr G.  Updates the model in place.
    -> (G list in parameters() order, carried hidden, [train losses], [validation losses])"""
    params = list(model.parameters())
    theta0 = [p.detach().clone() for p in params]
    w = task_weights(len(task_batches), ratio)
    G = [torch.zeros_like(p) for p in params]
    trl, val_l = [], []
    for i, (x, y) in enumerate(task_batches):
        out, hidden = model(x, detach(hidden))
        loss = F.cross_entropy(out.view(-1, out.size(2)), y)
        g_tr = [g.clone() for g in torch.autograd.grad(loss, params)]
        if clip:
            clip_(g_tr, clip)
        trl.append(float(loss.detach()))
        with torch.no_grad():
            for p, g in zip(params, g_tr):
                p.add_(g, alpha=-lr / meta_lr_factor)
        out, _ = model(val_batch[0], detach(hidden))
        vloss = F.cross_entropy(out.view(-1, out.size(2)), val_batch[1])
        val_l.append(float(vloss.detach()))
        g_val = torch.autograd.grad(vloss, params)
        with torch.no_grad():
            for acc, g in zip(G, g_val):
                acc.add_(g, alpha=w[i])
            for p, t0 in zip(params, theta0):
                p.copy_(t0)
    if clip:
        clip_(G, clip)
    with torch.no_grad():
        for p, g in zip(params, G):
            p.add_(g, alpha=-lr)
    return G, detach(hidden), trl, val_l
