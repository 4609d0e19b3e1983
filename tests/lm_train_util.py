"""Test helper (NOT product code): torch-CPU restatement of the reference's LM epoch loop (lm/main.py:256-277) and joint loop
(lm/main_joint.py:290-336) on tests/gru_ref.py's RNNModel, runnable in fp32 and fp64, pinned to the real reference by
tests/golden/LT0.npz (tests/test_lm_train.py); and `parent_epoch`, the same epoch composed from the library calls the project had
before mtl_lm_window_chains / mtl_sgd_clip_step (the bitwise yardstick of tests/test_lm_train_gpu.py and tools/bench_lm_train.py).
"""
import torch
import torch.nn.functional as F

from tests import gru_ref as GR


def schedule(S, bptt):
    return [(i, min(bptt, S - 1 - i)) for i in range(0, S - 1, bptt)]


def get_batch(source, i, bptt):
    T = min(bptt, len(source) - 1 - i)
    return source[i:i + T], source[i + 1:i + 1 + T].reshape(-1)


def clip_(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ (norm of the per-tensor norms; coefficient clamped to 1)"""
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    for g in grads:
        g.mul_(coef)


def sgd_(params, grads, lr, clip):
    grads = [g.clone() for g in grads]
    if clip:
        clip_(grads, clip)
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.add_(g, alpha=-lr)


def window_step(model, hidden, x, y, lr, clip):
    """one window of lm/main.py:258-275 -> (loss, new hidden (detached))"""
    params = list(model.parameters())
    out, hidden = model(x, GR.detach(hidden))
    loss = F.cross_entropy(out.view(-1, out.size(2)), y)
    sgd_(params, torch.autograd.grad(loss, params), lr, clip)
    return loss.detach(), GR.detach(hidden)


def epoch(model, stream, bptt, lr, clip, after=None):
    """-> ([losses], final hidden); after(w) is called after window w's update"""
    hidden = model.init_hidden(stream.shape[1])
    losses = []
    for w, (i, _) in enumerate(schedule(stream.shape[0], bptt)):
        x, y = get_batch(stream, i, bptt)
        loss, hidden = window_step(model, hidden, x, y, lr, clip)
        losses.append(loss)
        if after is not None:
            after(w)
    return losses, hidden


def joint_iteration(model, hidden, batches, lr, clip, ratio, reference_zero_grad=True):
    """one iteration of lm/main_joint.py:307-336 -> (sum w_i L_i, [L_i], hidden).  reference_zero_grad: model.zero_grad() before
    every task's forward (:271), so only the last task's weighted gradient reaches the step; False accumulates sum_i w_i g_i."""
    params = list(model.parameters())
    w = GR.task_weights(len(batches), ratio)
    G, losses = None, []
    for i, (x, y) in enumerate(batches):
        out, hidden = model(x, GR.detach(hidden))
        loss = F.cross_entropy(out.view(-1, out.size(2)), y)
        losses.append(loss.detach())
        g = torch.autograd.grad(loss * w[i], params)
        G = list(g) if (G is None or reference_zero_grad) else [a + b for a, b in zip(G, g)]
    sgd_(params, G, lr, clip)
    return sum(wi * float(li) for wi, li in zip(w, losses)), losses, GR.detach(hidden)


def flat(model):
    return torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()])


def load_flat(model, vec):
    off = 0
    with torch.no_grad():
        for _, p in model.named_parameters():
            p.copy_(vec[off:off + p.numel()].view_as(p).to(p.dtype))
            off += p.numel()
    assert off == vec.numel()


def parent_epoch(model, stream, bptt, lr, clip, log_interval=200):
    """The epoch LMTrainer.train_epoch runs, composed from what the project offered before it: per window g.zero_(),
    LMEngine.forward / backward (chains from LMEngine._chains), mtl_sumsq (mode 2), mtl_scale, mtl_axpy; the loss added to a device
    sum and read at the same log points.  `stream` (S, B) int64 on the device.  -> dict(losses (W,), hidden)"""
    import mtl_amd
    lib, check = mtl_amd._lib.lib(), mtl_amd._lib.check
    eng, theta = model.engine, model.flat_parameters
    dev = theta.device
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    g = torch.zeros_like(theta)
    coef = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(2048, dtype=torch.float32, device=dev)
    model.train()
    p = model.dropout_rate
    hidden = model.init_hidden(stream.shape[1])
    sched = schedule(stream.shape[0], bptt)
    losses = torch.zeros(len(sched), dtype=torch.float32, device=dev)
    total = torch.zeros(1, dtype=torch.float32, device=dev)
    n = theta.numel()
    for w, (i, T) in enumerate(sched):
        g.zero_()
        out = eng.forward(theta, stream[i:i + T], stream[i + 1:i + 1 + T].reshape(-1), hidden, p)
        hidden = out['hidden']
        eng.backward(g, 1.0)
        if clip:
            check(lib.mtl_sumsq(st(), g.data_ptr(), n, coef.data_ptr(), ws.data_ptr(), 2, float(clip)), 'mtl_sumsq')
            check(lib.mtl_scale(st(), g.data_ptr(), 1.0, coef.data_ptr(), n), 'mtl_scale')
        check(lib.mtl_axpy(st(), theta.data_ptr(), g.data_ptr(), -float(lr), n), 'mtl_axpy')
        losses[w:w + 1].copy_(out['loss'])
        total += out['loss']
        if w % log_interval == 0 and w > 0:
            eng.check_handoff()
            float(total)
            total.zero_()
    torch.cuda.synchronize(dev)
    eng.check_handoff()
    return dict(losses=losses, hidden=hidden)
