"""Utterances per second of the two ways from waveforms in host memory to a padded input batch on the device:

  (a) per utterance: K x `SpectrogramFrontEnd.__call__(y).cpu()`, `collate` on the host, `.to(device)`   (device_batches=False)
  (b) batched:       one `SpectrogramFrontEnd.batch(waves)`                                              (device_batches=True)

each on an idle device and while the default stream holds `--queued-ms` of queued kernels (a chain of matrix products enqueued right
before the timed call: the trainer's host thread runs up to two iterations ahead of the device, so the prefetch thread meets a
default stream with that much work in it).  K = 16 seeded ten-second waveforms (160 000 samples each), no disk.  A timed call ends
when its batch is complete on the device: (a) returns from a pageable host-to-device copy, which is synchronous; (b) waits on its
own event.  The host clock is read around each call, the device is drained (outside the timed span) between calls, the two paths
alternate, and the figure is the median of `--reps` calls after `--warmup`.  Also printed: the HIP-event time of the two launches of
mtl_spect_batch alone (operands already on the device).

    python tools/bench_frontend.py [--reps 20] [--warmup 3] [--queued-ms 100] [--out profiles/frontend_batch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def waveform(n, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return ((0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)) * np.linspace(0.2, 1.5, n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--utterances', type=int, default=16)
    ap.add_argument('--samples', type=int, default=160000)
    ap.add_argument('--queued-ms', type=float, default=100.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        ap.error('at least 20 timed calls after at least 3 warm-ups')
    assert torch.cuda.is_available(), 'bench_frontend.py measures on an MI355X'
    import mtl_amd
    from mtl_amd import _lib
    K = a.utterances
    waves = [waveform(a.samples, 100 + i) for i in range(K)]
    labels = [[4, 5]] * K
    fe = mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=True)
    dev = fe.device

    def per_utterance():
        specs = [fe(y).cpu() for y in waves]
        return mtl_amd.data.collate(specs, labels)[0].to(dev)

    def batched():
        return fe.batch(waves)[0]

    # the two paths must describe the same batch before their times are compared
    xa, xb = per_utterance(), batched()
    torch.cuda.synchronize()
    worst = max(float((xb[k].double() - xa[k].double()).norm() / xa[k].double().norm()) for k in range(K))
    assert xa.shape == xb.shape and worst < 2e-5, worst

    # the queued work of the busy case: products on the default stream, their number fitted to --queued-ms
    m = torch.randn(4096, 4096, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        m @ m
    e0.record()
    for _ in range(20):
        m @ m
    e1.record()
    torch.cuda.synchronize()
    chain = max(int(round(a.queued_ms / (e0.elapsed_time(e1) / 20))), 1)

    def timed(fn, busy):
        torch.cuda.synchronize()
        if busy:
            for _ in range(chain):
                m @ m
        t0 = time.perf_counter()
        x = fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        del x
        return dt

    times = {(name, busy): [] for name in ('per_utterance', 'batched') for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in (('per_utterance', per_utterance), ('batched', batched)):
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)

    # device time of the two launches alone
    lib = _lib.lib()
    flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves, fe.hop, fe.n_fft)
    d_wav, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
    out = torch.empty(K, 1, fe.F, tmax, device=dev)
    ws_bytes = lib.mtl_spect_batch_workspace(int(frames.sum()), K, fe.F)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    launch_us = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        e0.record()
        _lib.check(lib.mtl_spect_batch(st, d_wav.data_ptr(), d_off.data_ptr(), K, fe.n_fft, fe.hop, fe.basis.data_ptr(), fe.ldb, fe.F,
                                       out.data_ptr(), tmax, 1, ws.data_ptr(), ws_bytes), 'mtl_spect_batch')
        e1.record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            launch_us.append(1e3 * e0.elapsed_time(e1))

    def rate(key):
        return K / statistics.median(times[key])

    flop = 2.0 * int(frames.sum()) * 2 * fe.F * fe.n_fft
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=a.samples, frames_per_utterance=int(frames[0]),
               reps=a.reps, warmup=a.warmup, queued_ms=a.queued_ms, queued_products=chain, worst_rel_batched_vs_per_utterance=worst,
               utt_per_s=dict(per_utterance_idle=rate(('per_utterance', False)), batched_idle=rate(('batched', False)),
                              per_utterance_busy=rate(('per_utterance', True)), batched_busy=rate(('batched', True))),
               call_ms_median=dict(per_utterance_idle=1e3 * statistics.median(times[('per_utterance', False)]),
                                   batched_idle=1e3 * statistics.median(times[('batched', False)]),
                                   per_utterance_busy=1e3 * statistics.median(times[('per_utterance', True)]),
                                   batched_busy=1e3 * statistics.median(times[('batched', True)])),
               call_ms_min_max={'%s_%s' % (n, 'busy' if b else 'idle'): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               launches_us_median=statistics.median(launch_us), launches_us_min=min(launch_us),
               launches_gflop=flop / 1e9, launches_tflops=flop / (statistics.median(launch_us) * 1e-6) / 1e12)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
