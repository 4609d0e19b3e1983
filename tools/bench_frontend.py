"""Utterances per second of the two ways from waveforms in host memory to a padded input batch on the device (the
front-end classes and their `batch` are in frontend.py):

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

--noise-out PATH runs the noise-injection leg instead, same protocol, three paths that alternate:

  (a) clean:      `batch(waves)`
  (b) host mix:   the reference's mix (utils/data_loader.py:396-398) in numpy on the calling thread, then `batch(mixed)`
  (c) device mix: `batch(waves, noise=plan)`, every utterance noisy

over a seeded noise corpus of four 30-second files written to a temporary directory, plus the HIP-event times of mtl_spect_batch,
mtl_spect_batch_noise and mtl_wave_mix_coef alone.

    python tools/bench_frontend.py --noise-out profiles/frontend_noise.json

--augment [--augment-out PATH] runs the tempo / gain leg instead, same protocol, three paths that alternate:

  (a) clean:         `batch(waves)`
  (b) per utterance: K x `__call__(y).cpu()`, `collate`, `.to(device)`  (the figure an augmented batch must stay under to be worth it)
  (c) augmented:     `batch(waves, augment=(tempo, gain_db))`, every utterance stretched (seeded draws of TempoGainAugment)

plus the HIP-event times of mtl_tempo_search, mtl_tempo_render and of mtl_spect_batch on the stretched buffer alone.

    python tools/bench_frontend.py --augment --augment-out profiles/frontend_augment.json

--resample [--resample-out PATH] runs the rate-conversion leg instead, same protocol, three paths that alternate over
K = 16 ten-second utterances at 8 kHz (80 000 samples each) for a 16 kHz front-end:

  (a) device:   `batch(waves, rates=[8000] * K)`
  (b) host:     `scipy.signal.resample_poly(y, 2, 1)` per utterance on the calling thread, then `batch(converted)`: what a user does today
  (c) at rate:  `batch` of audio that is at 16 kHz already, of the same output length (the floor: no conversion at all)

plus the HIP-event time of mtl_resample alone and the bytes it reads and writes over that time, against the HBM rate.

    python tools/bench_frontend.py --resample --resample-out profiles/frontend_resample.json

--logfbank [--logfbank-out PATH] runs the log-mel filterbank leg instead, same protocol, four paths that alternate
over the K waveforms rounded to 16-bit values:

  (a) batched:       one `LogFBankFrontEnd.batch(waves)`
  (b) per utterance: K x `LogFBankFrontEnd.__call__(y).cpu()`, `collate`, `.to(device)`
  (c) host:          the fp64 numpy restatement of the features per utterance on the calling thread, `collate`, `.to(device)`: what a
                     user who wants the 80-band input does today
  (d) spectrogram:   `SpectrogramFrontEnd.batch(waves)` on the same waveforms (161 bins)

plus the HIP-event times of the two launches of mtl_fbank_batch and of mtl_spect_batch alone (operands already on the device).

    python tools/bench_frontend.py --logfbank --logfbank-out profiles/frontend_logfbank.json

--specaug [--specaug-out PATH] runs the SpecAugment leg instead, same protocol, two paths that alternate, for the
spectrogram and for the log-mel filterbank front-end:

  (a) clean:     `batch(waves)`
  (b) augmented: `batch(waves, spec=table)`, the default policy (W = 40, two frequency masks of up to 27 rows, two time masks of up to 40
                 frames), seeded draws (an utterance whose draw gives w == c is not warped: `warped_utterances` counts the others)

plus the HIP-event time of mtl_spec_augment alone on a finished batch and the bytes it reads and writes over that time (a warped row is
read and written over [0, tau), a frequency-masked row written, any other row written over its time spans), against the HBM rate.

    python tools/bench_frontend.py --specaug --specaug-out profiles/frontend_specaug.json
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
    ap.add_argument('--noise-out', default=None)
    ap.add_argument('--augment', action='store_true')
    ap.add_argument('--augment-out', default=None)
    ap.add_argument('--resample', action='store_true')
    ap.add_argument('--resample-out', default=None)
    ap.add_argument('--logfbank', action='store_true')
    ap.add_argument('--logfbank-out', default=None)
    ap.add_argument('--specaug', action='store_true')
    ap.add_argument('--specaug-out', default=None)
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
    if a.noise_out:
        return noise_leg(a, mtl_amd, _lib, fe, waves)
    if a.augment or a.augment_out:
        return augment_leg(a, mtl_amd, _lib, fe, waves, labels)
    if a.resample or a.resample_out:
        return resample_leg(a, mtl_amd, _lib, fe, waves)
    if a.logfbank or a.logfbank_out:
        return logfbank_leg(a, mtl_amd, _lib, fe, waves, labels)
    if a.specaug or a.specaug_out:
        return specaug_leg(a, mtl_amd, _lib, fe, waves)

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


def noise_leg(a, mtl_amd, _lib, fe, waves):
    import tempfile
    import wave
    K, dev = len(waves), fe.device
    with tempfile.TemporaryDirectory() as d:
        for i in range(4):
            with wave.open(os.path.join(d, 'noise%d.wav' % i), 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes((np.clip(waveform(3 * a.samples, 900 + i)[::-1], -1, 1) * 32767).astype('<i2').tobytes())
        inj = mtl_amd.NoiseInjection(d, 16000, (0.1, 0.5))
    rng = np.random.RandomState(1)
    plan = inj.plan([inj.draw(rng, 1.0) for _ in range(K)], [len(y) for y in waves])
    assert (plan[0] >= 0).all()

    def clean():
        return fe.batch(waves)[0]

    def host_mix():
        mixed = []
        for y, o, lv in zip(waves, plan[0], plan[1]):
            n = inj.bank[o:o + len(y)].astype(np.float32) / np.float32(32768.0)
            noise_energy, data_energy = np.sqrt(n.dot(n) / n.size), np.sqrt(y.dot(y) / y.size)
            mixed.append(y + lv * n * data_energy / noise_energy)
        return fe.batch(mixed)[0]

    def device_mix():
        return fe.batch(waves, noise=(inj,) + plan)[0]

    xa, xb, xc = clean(), host_mix(), device_mix()
    torch.cuda.synchronize()
    worst = max(float((xc[k].double() - xb[k].double()).norm() / xb[k].double().norm()) for k in range(K))
    moved = min(float((xc[k].double() - xa[k].double()).norm() / xa[k].double().norm()) for k in range(K))
    assert xb.shape == xc.shape and worst < 2e-5 and moved > 1e-3, (worst, moved)

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

    paths = (('clean', clean), ('host_mix', host_mix), ('device_mix', device_mix))
    times = {(name, busy): [] for name, _ in paths for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in paths:
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)

    # device time of the launches alone (operands on the device)
    lib = _lib.lib()
    flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves, fe.hop, fe.n_fft)
    d_wav, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
    d_noff, d_lvl = torch.from_numpy(plan[0]).to(dev), torch.from_numpy(plan[1]).to(dev)
    bank, coef = inj.device_bank(), torch.empty(K, device=dev)
    out = torch.empty(K, 1, fe.F, tmax, device=dev)
    ws_bytes, cws_bytes = lib.mtl_spect_batch_workspace(int(frames.sum()), K, fe.F), lib.mtl_wave_mix_coef_workspace(K)
    ws, cws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev), torch.empty(cws_bytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    spect = (st, d_wav.data_ptr(), d_off.data_ptr(), K, fe.n_fft, fe.hop, fe.basis.data_ptr(), fe.ldb, fe.F, out.data_ptr(), tmax, 1,
             ws.data_ptr(), ws_bytes)
    calls = dict(
        spect_batch=lambda: lib.mtl_spect_batch(*spect),
        wave_mix_coef=lambda: lib.mtl_wave_mix_coef(st, d_wav.data_ptr(), d_off.data_ptr(), K, bank.data_ptr(), inj.bank_len, d_noff.data_ptr(),
                                                    d_lvl.data_ptr(), coef.data_ptr(), cws.data_ptr(), cws_bytes),
        spect_batch_noise=lambda: lib.mtl_spect_batch_noise(*(spect + (bank.data_ptr(), inj.bank_len, d_noff.data_ptr(), coef.data_ptr()))))
    launch_us = {name: [] for name in calls}
    for rep in range(a.warmup + a.reps):
        for name in ('wave_mix_coef', 'spect_batch', 'spect_batch_noise'):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(calls[name](), name)
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                launch_us[name].append(1e3 * e0.elapsed_time(e1))

    key = lambda n, b: '%s_%s' % (n, 'busy' if b else 'idle')
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=a.samples, reps=a.reps, warmup=a.warmup,
               queued_ms=a.queued_ms, queued_products=chain, bank_samples=inj.bank_len, worst_rel_device_vs_host_mix=worst,
               least_rel_noisy_vs_clean=moved,
               utt_per_s={key(n, b): K / statistics.median(v) for (n, b), v in times.items()},
               call_ms_median={key(n, b): 1e3 * statistics.median(v) for (n, b), v in times.items()},
               call_ms_min_max={key(n, b): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               launches_us_median={n: statistics.median(v) for n, v in launch_us.items()},
               launches_us_min={n: min(v) for n, v in launch_us.items()})
    print(json.dumps(res))
    with open(a.noise_out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')


def augment_leg(a, mtl_amd, _lib, fe, waves, labels):
    K, dev = len(waves), fe.device
    waves = [(np.rint(y.astype(np.float64) * 32768.0) / 32768.0).astype(np.float32) for y in waves]      # what a 16-bit file holds
    aug, rng = mtl_amd.TempoGainAugment(), np.random.RandomState(1)
    tempo, gain_db, out_lengths = aug.plan([aug.draw(rng) for _ in range(K)], [len(y) for y in waves])
    assert (tempo != 1.0).all()

    def clean():
        return fe.batch(waves)[0]

    def per_utterance():
        specs = [fe(y).cpu() for y in waves]
        return mtl_amd.data.collate(specs, labels)[0].to(dev)

    def augmented():
        return fe.batch(waves, augment=(tempo, gain_db))[0]

    # the augmented batch must be the batch of the unfused form's waveforms before its time means anything
    stretched, seg_off = fe.tempo_gain(waves, tempo, gain_db)
    xa, xc = fe.batch(stretched)[0], augmented()
    torch.cuda.synchronize()
    assert [len(s) for s in stretched] == out_lengths.tolist() and torch.equal(xa, xc)

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

    paths = (('clean', clean), ('per_utterance', per_utterance), ('augmented', augmented))
    times = {(name, busy): [] for name, _ in paths for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in paths:
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)

    # device time of the launches alone (operands on the device)
    lib = _lib.lib()
    tab = mtl_amd.tempo_gain_tables(waves, tempo, gain_db, 16000)
    S, R, O = tab['geometry']
    d = {k: torch.from_numpy(tab[k]).to(dev) for k in ('flat', 'offsets', 'out_offsets', 'seg_base', 'tempo', 'gain')}
    seg = torch.empty(int(tab['seg_base'][-1]), dtype=torch.int32, device=dev)
    d_str = torch.empty(int(tab['out_offsets'][-1]), device=dev)
    frames = 1 + np.diff(tab['out_offsets']) // fe.hop
    tmax = int(frames.max())
    out = torch.empty(K, 1, fe.F, tmax, device=dev)
    ws_bytes = lib.mtl_spect_batch_workspace(int(frames.sum()), K, fe.F)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    head = (st, d['flat'].data_ptr(), d['offsets'].data_ptr(), d['out_offsets'].data_ptr(), d['tempo'].data_ptr())
    calls = dict(
        tempo_search=lambda: lib.mtl_tempo_search(*(head + (d['seg_base'].data_ptr(), K, S, R, O, seg.data_ptr()))),
        tempo_render=lambda: lib.mtl_tempo_render(*(head + (d['gain'].data_ptr(), d['seg_base'].data_ptr(), seg.data_ptr(), K, S, R, O, 1,
                                                            d_str.data_ptr()))),
        spect_batch=lambda: lib.mtl_spect_batch(st, d_str.data_ptr(), d['out_offsets'].data_ptr(), K, fe.n_fft, fe.hop, fe.basis.data_ptr(),
                                                fe.ldb, fe.F, out.data_ptr(), tmax, 1, ws.data_ptr(), ws_bytes))
    launch_us = {name: [] for name in calls}
    for rep in range(a.warmup + a.reps):
        for name in ('tempo_search', 'tempo_render', 'spect_batch'):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(calls[name](), name)
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                launch_us[name].append(1e3 * e0.elapsed_time(e1))
    assert torch.equal(seg.cpu(), torch.from_numpy(seg_off))

    key = lambda n, b: '%s_%s' % (n, 'busy' if b else 'idle')
    segments = np.diff(tab['seg_base'])
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=a.samples, reps=a.reps, warmup=a.warmup,
               queued_ms=a.queued_ms, queued_products=chain, tempo_min_max=[float(tempo.min()), float(tempo.max())],
               stretched_samples_min_max=[int(out_lengths.min()), int(out_lengths.max())],
               segments_per_utterance_min_max=[int(segments.min()), int(segments.max())],
               utt_per_s={key(n, b): K / statistics.median(v) for (n, b), v in times.items()},
               call_ms_median={key(n, b): 1e3 * statistics.median(v) for (n, b), v in times.items()},
               call_ms_min_max={key(n, b): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               launches_us_median={n: statistics.median(v) for n, v in launch_us.items()},
               launches_us_min={n: min(v) for n, v in launch_us.items()},
               search_us_per_link=statistics.median(launch_us['tempo_search']) / max(int(segments.max()) - 1, 1))
    print(json.dumps(res))
    if a.augment_out:
        with open(a.augment_out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


HBM_TBPS = 8.0          # MI355X: 8 TB/s of HBM3E bandwidth (the vendor's figure)


def resample_leg(a, mtl_amd, _lib, fe, waves16):
    from scipy.signal import resample_poly
    K, dev, rate = len(waves16), fe.device, 8000
    # ten seconds at 8 kHz, as a 16-bit file holds them; the 16 kHz audio of path (c) has the length that the conversion gives
    waves = [(np.rint(y[::2].astype(np.float64) * 32768.0) / 32768.0).astype(np.float32) for y in waves16]
    rates = [rate] * K
    out_lengths = mtl_amd.resample_plan([len(y) for y in waves], rates, fe.sample_rate)[0]
    at_rate = [y[:n] for y, n in zip(waves16, out_lengths)]
    assert [len(y) for y in at_rate] == out_lengths.tolist()

    def device():
        return fe.batch(waves, rates=rates)[0]

    def host():
        return fe.batch([resample_poly(y, 2, 1).astype(np.float32) for y in waves])[0]

    def same_length():
        return fe.batch(at_rate)[0]

    # the converted batch must be the batch of the unfused form's waveforms, and close to the host's, before its time means anything
    converted = fe.resample(waves, rates)
    xa, xb, xc = device(), host(), fe.batch(converted)[0]
    torch.cuda.synchronize()
    assert [len(c) for c in converted] == out_lengths.tolist() and torch.equal(xa, xc) and xa.shape == xb.shape
    vs_host = max(float((xa[k].double() - xb[k].double()).norm() / xb[k].double().norm()) for k in range(K))

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

    paths = (('device', device), ('host', host), ('at_rate', same_length))
    times = {(name, busy): [] for name, _ in paths for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in paths:
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)
    host_convert_ms = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        [resample_poly(y, 2, 1).astype(np.float32) for y in waves]
        if rep >= a.warmup:
            host_convert_ms.append(1e3 * (time.perf_counter() - t0))

    # device time of the launch alone (operands on the device)
    lib = _lib.lib()
    tab = mtl_amd.resample_tables(waves, rates, fe.sample_rate)
    d = {k: torch.from_numpy(tab[k]).to(dev) for k in ('flat', 'offsets', 'out_offsets', 'plan', 'taps')}
    d_out = torch.empty(int(tab['out_offsets'][-1]), device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    launch_us = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        e0.record()
        _lib.check(lib.mtl_resample(st, d['flat'].data_ptr(), d['offsets'].data_ptr(), d['out_offsets'].data_ptr(), d['plan'].data_ptr(),
                                    d['taps'].data_ptr(), tab['taps'].shape[0], K, 1, d_out.data_ptr()), 'mtl_resample')
        e1.record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            launch_us.append(1e3 * e0.elapsed_time(e1))
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate(converted))
    moved = 4 * tab['flat'].shape[0] + 4 * d_out.numel() + 8 * tab['taps'].shape[0] + 8 * (2 * (K + 1) + 4 * K)
    terms = int(tab['out_offsets'][-1]) * (tab['taps'].shape[0] // int(tab['plan'][0, 0]) + 1)
    tbps = moved / (statistics.median(launch_us) * 1e-6) / 1e12

    key = lambda n, b: '%s_%s' % (n, 'busy' if b else 'idle')
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=len(waves[0]), rate_in=rate, rate_out=fe.sample_rate,
               converted_samples_per_utterance=int(out_lengths[0]), taps=int(tab['taps'].shape[0]), reps=a.reps, warmup=a.warmup,
               queued_ms=a.queued_ms, queued_products=chain, worst_rel_device_vs_host_features=vs_host,
               utt_per_s={key(n, b): K / statistics.median(v) for (n, b), v in times.items()},
               call_ms_median={key(n, b): 1e3 * statistics.median(v) for (n, b), v in times.items()},
               call_ms_min_max={key(n, b): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               host_resample_poly_ms_median=statistics.median(host_convert_ms),
               launch_us_median=statistics.median(launch_us), launch_us_min=min(launch_us), launch_bytes=moved,
               launch_tb_per_s=tbps, hbm_tb_per_s=HBM_TBPS, launch_share_of_hbm_rate=tbps / HBM_TBPS,
               launch_fp64_gflops=2.0 * terms / (statistics.median(launch_us) * 1e-6) / 1e9)
    print(json.dumps(res))
    if a.resample_out:
        with open(a.resample_out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


HBM_ACHIEVABLE_TBPS = 6.3          # what a streaming copy reaches of the 8 TB/s (DESIGN.md section 21 quotes the same figure)


def specaug_bytes(table, F, freq_masks, time_masks):
    """the bytes that mtl_spec_augment moves for this table: per (utterance, row) 4 tau written under a frequency mask, else 8 tau (read and
    written) when warped, else 4 per frame under a time mask"""
    total = 0
    for row in np.asarray(table):
        tau, c, w = (int(v) for v in row[:3])
        rows = np.zeros(F, dtype=bool)
        for m in range(freq_masks):
            rows[row[3 + 2 * m]:row[3 + 2 * m] + row[4 + 2 * m]] = True
        cols = np.zeros(tau, dtype=bool)
        for m in range(time_masks):
            t0, t = row[3 + 2 * freq_masks + 2 * m], row[4 + 2 * freq_masks + 2 * m]
            cols[t0:t0 + t] = True
        total += int(rows.sum()) * 4 * tau + int((~rows).sum()) * (8 * tau if w != c else 4 * int(cols.sum()))
    return total


def specaug_leg(a, mtl_amd, _lib, fe, waves):
    K, dev = len(waves), fe.device
    sa = mtl_amd.SpecAugment()
    fes = dict(spectrogram=fe, logfbank=mtl_amd.LogFBankFrontEnd(16000, 80, normalize=True))
    rng = np.random.RandomState(23)
    draws = [sa.draw(rng) for _ in range(K)]
    tables = {}
    for name, f in fes.items():
        clean, sizes = f.batch(waves)
        tables[name] = sa.plan(draws, sizes.numpy(), f.F)
        got = f.batch(waves, spec=tables[name])[0]
        torch.cuda.synchronize()
        assert got.shape == clean.shape and not torch.equal(got, clean) and bool(torch.isfinite(got).all())
        del clean, got

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

    paths = []
    for name, f in fes.items():
        paths.append((name + '_clean', lambda f=f: f.batch(waves)[0]))
        paths.append((name + '_specaug', lambda f=f, t=tables[name]: f.batch(waves, spec=t)[0]))
    times = {(name, busy): [] for name, _ in paths for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in paths:
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)

    # device time of the launch alone, on a finished batch (in place: every repetition moves the same bytes)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    launch = {}
    for name, f in fes.items():
        x = f.batch(waves)[0]
        t = tables[name]
        d_t = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
        us = []
        for rep in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(lib.mtl_spec_augment(st, x.data_ptr(), K, f.F, x.size(3), d_t.data_ptr(), t.freq_masks, t.time_masks), 'mtl_spec_augment')
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                us.append(1e3 * e0.elapsed_time(e1))
        moved = specaug_bytes(t, f.F, t.freq_masks, t.time_masks)
        tbps = moved / (statistics.median(us) * 1e-6) / 1e12
        launch[name] = dict(launch_us_median=statistics.median(us), launch_us_min=min(us), launch_bytes=moved, batch_bytes=4 * x.numel(),
                            launch_tb_per_s=tbps, launch_share_of_hbm_rate=tbps / HBM_TBPS, launch_share_of_achievable_hbm_rate=tbps / HBM_ACHIEVABLE_TBPS, rows=f.F,
                            frames=int(x.size(3)), warped_utterances=int((t[:, 1] != t[:, 2]).sum()))

    key = lambda n, b: '%s_%s' % (n, 'busy' if b else 'idle')
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=len(waves[0]), reps=a.reps, warmup=a.warmup,
               queued_ms=a.queued_ms, queued_products=chain, policy=dict(time_warp=sa.time_warp, freq_masks=sa.freq_masks,
                                                                         freq_width=sa.freq_width, time_masks=sa.time_masks,
                                                                         time_width=sa.time_width, time_ratio=sa.time_ratio),
               utt_per_s={key(n, b): K / statistics.median(v) for (n, b), v in times.items()},
               call_ms_median={key(n, b): 1e3 * statistics.median(v) for (n, b), v in times.items()},
               call_ms_min_max={key(n, b): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               hbm_tb_per_s=HBM_TBPS, hbm_achievable_tb_per_s=HBM_ACHIEVABLE_TBPS, launch=launch)
    print(json.dumps(res))
    if a.specaug_out:
        with open(a.specaug_out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


def logfbank_leg(a, mtl_amd, _lib, fe, waves, labels):
    K, dev = len(waves), fe.device
    waves = [(np.rint(y.astype(np.float64) * 32768.0) / 32768.0).astype(np.float32) for y in waves]      # what a 16-bit file holds
    fb = mtl_amd.LogFBankFrontEnd(fe.sample_rate, 80, normalize=True)
    table = fb.filterbank

    def host_features(y):
        """the definition in fp64 numpy, normalised"""
        s = 32768.0 * y.astype(np.float64)
        p = s.copy()
        p[1:] -= 0.97 * s[:-1]
        T = int(mtl_amd.fbank_frames([len(y)], fe.sample_rate)[0])
        padded = np.zeros((T - 1) * fb.fs + fb.fl)
        padded[:len(p)] = p
        frames = np.lib.stride_tricks.as_strided(padded, (T, fb.fl), (padded.strides[0] * fb.fs, padded.strides[0]))
        spec = np.fft.rfft(frames, fb.nfft, axis=1)
        E = table @ ((spec.real ** 2 + spec.imag ** 2) / fb.nfft).T
        v = np.log(np.where(E == 0, mtl_amd.data.FBANK_EPS, E))
        return torch.from_numpy(((v - v.mean()) / v.std(ddof=1)).astype(np.float32))

    def batched():
        return fb.batch(waves)[0]

    def per_utterance():
        return mtl_amd.data.collate([fb(y).cpu() for y in waves], labels)[0].to(dev)

    def host():
        return mtl_amd.data.collate([host_features(y) for y in waves], labels)[0].to(dev)

    def spectrogram():
        return fe.batch(waves)[0]

    # the three filterbank paths must describe the same batch before their times are compared
    xa, xb, xc = batched(), per_utterance(), host()
    torch.cuda.synchronize()
    assert xa.shape == xb.shape == xc.shape == (K, 1, 80, int(mtl_amd.fbank_frames([len(waves[0])], fe.sample_rate)[0])) and torch.equal(xa, xb)
    vs_host = float((xa.double() - xc.double()).abs().max())              # (the largest is an ill-conditioned element: band 0, the DC bin)
    vs_host_l2 = float((xa.double() - xc.double()).norm() / xc.double().norm())
    assert vs_host_l2 < 1e-4, vs_host_l2

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

    paths = (('batched', batched), ('per_utterance', per_utterance), ('host', host), ('spectrogram', spectrogram))
    times = {(name, busy): [] for name, _ in paths for busy in (False, True)}
    for rep in range(a.warmup + a.reps):
        for busy in (False, True):
            for name, fn in paths:
                dt = timed(fn, busy)
                if rep >= a.warmup:
                    times[(name, busy)].append(dt)
    host_features_ms = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        [host_features(y) for y in waves]
        if rep >= a.warmup:
            host_features_ms.append(1e3 * (time.perf_counter() - t0))

    # device time of the launches alone (operands on the device): the new kernel, and the spectrogram's on the same samples
    lib = _lib.lib()
    flat, offsets = np.concatenate(waves), np.concatenate([[0], np.cumsum([len(y) for y in waves])]).astype(np.int64)
    frames = mtl_amd.fbank_frames([len(y) for y in waves], fe.sample_rate).astype(np.int32)
    tmax = int(frames.max())
    d_wav, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
    out = torch.empty(K, 1, 80, tmax, device=dev)
    ws_bytes = lib.mtl_fbank_batch_workspace(K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    _, _, sframes, stmax = mtl_amd.pack_waveforms(waves, fe.hop, fe.n_fft)
    sout = torch.empty(K, 1, fe.F, stmax, device=dev)
    sws_bytes = lib.mtl_spect_batch_workspace(int(sframes.sum()), K, fe.F)
    sws = torch.empty(sws_bytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def fbank_launch():
        _lib.check(lib.mtl_fbank_batch(st, d_wav.data_ptr(), d_off.data_ptr(), K, fb.fl, fb.fs, fb.nfft, fb.basis.data_ptr(), fb.ldb, fb.nfilt,
                                       fb.band.data_ptr(), fb.band_w.data_ptr(), fb.band_w.numel(), out.data_ptr(), tmax, 1, ws.data_ptr(),
                                       ws_bytes), 'mtl_fbank_batch')

    def spect_launch():
        _lib.check(lib.mtl_spect_batch(st, d_wav.data_ptr(), d_off.data_ptr(), K, fe.n_fft, fe.hop, fe.basis.data_ptr(), fe.ldb, fe.F,
                                       sout.data_ptr(), stmax, 1, sws.data_ptr(), sws_bytes), 'mtl_spect_batch')
    launch_us = {'fbank': [], 'spect': []}
    for rep in range(a.warmup + a.reps):
        for name, fn in (('fbank', fbank_launch), ('spect', spect_launch)):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                launch_us[name].append(1e3 * e0.elapsed_time(e1))
    assert torch.equal(out, xa)

    key = lambda n, b: '%s_%s' % (n, 'busy' if b else 'idle')
    flop = 2.0 * int(frames.sum()) * 2 * (fb.nfft // 2 + 1) * fb.fl
    res = dict(device=torch.cuda.get_device_name(0), utterances=K, samples_per_utterance=len(waves[0]), frames_per_utterance=int(frames[0]),
               spectrogram_frames_per_utterance=int(sframes[0]), reps=a.reps, warmup=a.warmup, queued_ms=a.queued_ms, queued_products=chain,
               batched_equals_per_utterance=True, worst_abs_batched_vs_host_fp64_normalised=vs_host, rel_l2_batched_vs_host_fp64_normalised=vs_host_l2,
               utt_per_s={key(n, b): K / statistics.median(v) for (n, b), v in times.items()},
               call_ms_median={key(n, b): 1e3 * statistics.median(v) for (n, b), v in times.items()},
               call_ms_min_max={key(n, b): [1e3 * min(v), 1e3 * max(v)] for (n, b), v in times.items()},
               host_features_ms_median=statistics.median(host_features_ms),
               fbank_launches_us_median=statistics.median(launch_us['fbank']), fbank_launches_us_min=min(launch_us['fbank']),
               spect_launches_us_median=statistics.median(launch_us['spect']), spect_launches_us_min=min(launch_us['spect']),
               fbank_dft_gflop=flop / 1e9, fbank_dft_tflops=flop / (statistics.median(launch_us['fbank']) * 1e-6) / 1e12,
               output_elements=dict(logfbank=int(out.numel()), spectrogram=int(sout.numel())))
    print(json.dumps(res))
    if a.logfbank_out:
        with open(a.logfbank_out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
