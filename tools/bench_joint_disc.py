"""Joint training with the accent discriminator at the north-star size (8 tasks x 8 utterances x 1000 frames x 100 labels, enc2/dec4
d512): what the head costs per iteration, and its two kernel calls against the same computation written with torch ops.

In ONE process, interleaved, medians after a warm-up:
  (a) JointTrainer.run_iteration with discriminator=None, (b) --multitask, (c) --adversarial           (host clock around a device sync)
  the HIP pair mtl_disc_fwd + mtl_disc_bwd on a (B, T', d) encoder output, and torch's sum -> F.linear -> cross_entropy / mse_loss ->
  autograd into a denc tensor added by mtl_axpy (+ the two parameter-gradient accumulations)                              (HIP events)

    python tools/bench_joint_disc.py --out profiles/joint_discriminator.json
    python tools/bench_joint_disc.py --root <checkout of another revision> --baseline-only --out parent.json      # (a) alone, on that
        revision's package (the parent commit has no discriminator); --parent-json parent.json ... records those runs next to this one's
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=HERE, help='repository root whose package is measured')
    ap.add_argument('--baseline-only', action='store_true', help='only (a): uses nothing but the discriminator-free trainer API')
    ap.add_argument('--tasks', type=int, default=8)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--labels', type=int, default=100)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--num-class', type=int, default=8)
    ap.add_argument('--kernel-reps', type=int, default=200)
    ap.add_argument('--parent-json', nargs='*', default=[])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import bench                                    # the flagship configuration (CFG, make_args) of the measured revision
    import mtl_amd
    assert torch.cuda.is_available(), 'needs an MI355X: there is nothing to measure without one'
    dev = torch.device('cuda:0')
    args = bench.make_args(a.k)
    args.lr, args.lr_disc, args.num_class, args.beta_decay = 1e-4, 1e-4, a.num_class, False
    vocab = mtl_amd.synthetic_vocab(bench.CFG['vocab_size'])
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=bench.CFG['r']).cuda()
    model.train()
    n = a.tasks
    tasks = [mtl_amd.SyntheticTask(m, a.k, a.frames, a.labels, bench.CFG['vocab_size'], variable=False) for m in range(n)]
    batches = [t.sample(a.k, 1, m)[0] for m, t in enumerate(tasks)]
    batches = [(b[0].cuda(), b[1], b[2], b[3], b[4]) for b in batches]
    tr = mtl_amd.JointTrainer()
    opt = mtl_amd.FlatAdam(model, args.lr)
    variants = {'none': {}}
    if not a.baseline_only:
        disc = mtl_amd.init_discriminator_model(args).cuda()
        opt_disc = torch.optim.Adam(disc.parameters(), lr=args.lr_disc)
        variants['multitask'] = dict(discriminator=disc, opt_disc=opt_disc, flags=(False, True))
        variants['adversarial'] = dict(discriminator=disc, opt_disc=opt_disc, flags=(True, False))

    def iteration(name):
        kw = dict(variants[name])
        if 'flags' in kw:
            args.adversarial, args.multitask = kw.pop('flags')
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tr.run_iteration(model, vocab, batches, n, opt, args, **kw)        # (ends in a device synchronise)
        return (time.perf_counter() - t0) * 1e3

    times = {name: [] for name in variants}
    for step in range(a.warmup + a.steps):
        for name in variants:                                              # interleaved: a, b, c, a, b, c, ...
            ms = iteration(name)
            if step >= a.warmup:
                times[name].append(ms)
    out = dict(config=dict(tasks=n, k=a.k, frames=a.frames, labels=a.labels, steps=a.steps, warmup=a.warmup, num_class=a.num_class,
                           baseline_only=bool(a.baseline_only)),
               iteration_ms={name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in times.items()})

    if not a.baseline_only:
        import torch.nn.functional as F
        lib = mtl_amd._lib.lib()
        B, T4, d, C = a.k, a.frames // 4, bench.CFG['dim_model'], a.num_class
        enc = torch.randn(B, T4, d, device=dev)
        denc = torch.zeros(B * T4, d, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def hip_pair(adv):
            disc.head_forward(enc, 3 % C, adv)
            disc.head_backward(0.5 / n, 1.0 / n if adv else 0.0, denc)

        W, bias = disc.linear.weight, disc.linear.bias
        tgt = torch.full((B,), 3 % C, dtype=torch.long, device=dev)
        uniform = torch.full((B, C), 1.0 / C, device=dev)

        def torch_pair(adv):
            e = enc.detach().requires_grad_(True)
            w, b_ = W.detach().requires_grad_(True), bias.detach().requires_grad_(True)
            logits = F.linear(e.sum(dim=1), w, b_)
            loss = (0.5 / n) * F.cross_entropy(logits, tgt)
            if adv:
                loss = loss + (1.0 / n) * F.mse_loss(logits, uniform)
            ge, gw, gb = torch.autograd.grad(loss, [e, w, b_])
            mtl_amd._lib.check(lib.mtl_axpy(st, denc.data_ptr(), ge.contiguous().data_ptr(), 1.0, denc.numel()), 'mtl_axpy')
            W.grad.add_(gw)
            bias.grad.add_(gb)

        def timed(fn, adv):
            for _ in range(10):
                fn(adv)
            ms = []
            for _ in range(a.kernel_reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(adv)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) * 1e3)
            return dict(median_us=statistics.median(ms), min_us=min(ms))
        kern = {}
        for adv in (False, True):                                          # alternating HIP / torch, twice
            tag = 'adversarial' if adv else 'multitask'
            kern[tag] = dict(hip=timed(hip_pair, adv), torch=timed(torch_pair, adv))
            kern[tag]['hip_again'] = timed(hip_pair, adv)
        # bytes the head must move: one read of enc, one read-modify-write of denc
        out['head'] = dict(shape=dict(B=B, T=T4, d=d, C=C), event_us=kern, min_bytes=3 * 4 * B * T4 * d)
    if a.parent_json:
        out['parent_runs'] = [json.load(open(p)) for p in a.parent_json]
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
