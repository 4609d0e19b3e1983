// Sample-rate conversion for gfx950 (MI355X) in front of the tempo stage of the batched spectrogram front-end (audio_with_sox and
// augment_audio_with_sox, utils/audio.py: `sox -r`).  What sox did is pinned by a definition of ours (DESIGN.md section 14,
// tests/resample_util.py), parity with sox unpinned:
//
//   ratio   g = gcd(r_in, r_out), up = r_out / g, down = r_in / g; utterance k of L samples becomes N = ceil(L up / down) samples (the
//           out_offsets table is the host's).  up == down (== 1) bypasses the filter: a copy, bit for bit.
//   taps    h, 2 half + 1 doubles per distinct (up, down), formed on the host (a Kaiser-windowed sinc, sum(h) == up) and read as uploaded.
//   output  y[j] = sum_i x[i] h[j down - i up + half] over 0 <= i < L with the tap index in [0, 2 half]: zero-phase, zero extension.
//           fp64, one fma per term, in ascending i.
//   file    then clip(rint(y 32768), -32768, 32767) / 32768 formed in fp64 and rounded once to fp32 (exact): the 16-bit file without dither.
//
//   mtl_resample   grid over (utterance, slot) like wave_mix_kernel: every output sample from the samples, the plan and the taps alone.
//                  The terms of output j are i in [ceil((j down - half) / up), floor((j down + half) / up)] cut to [0, L): the loop bounds
//                  ARE the guards of the sample reads and of the tap reads; that an utterance's table lies inside `taps` is checked once
//                  per workgroup.  j down and every offset are 64-bit.  Neighbouring lanes read neighbouring samples and taps `down`
//                  apart: both stay in the caches (the longest table allowed, 2 * 16 * 1024 + 1 doubles, is 256 KiB), no LDS staging.
// No atomics, no workspace: bitwise repeatable.
#include "mtl_common.h"

namespace {

constexpr int RS_TARGET_GROUPS = 2048;   // workgroups of a launch, about: slots per utterance = ceil(RS_TARGET_GROUPS / K) in [1, 256]
constexpr long RS_MAX_RATIO = 1024;      // max(up, down) the host accepts; a plan beyond it writes zeros

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ wav, const long* __restrict__ offsets,
                                                       const long* __restrict__ out_offsets, const long* __restrict__ plan,
                                                       const double* __restrict__ taps, long n_taps, int K, int slots, int quantize,
                                                       float* __restrict__ out) {
    const int k = blockIdx.x % K, slot = blockIdx.x / K;
    const long off = offsets[k];
    const long L = offsets[k + 1] - off;
    const long ooff = out_offsets[k];
    const long N = out_offsets[k + 1] - ooff;
    const long up = plan[4 * k], down = plan[4 * k + 1], half = plan[4 * k + 2], base = plan[4 * k + 3];
    const float* x = wav + off;
    const long stride = 256L * slots;
    if (up == down) {                                                     // the bypass (uniform over the workgroup)
        for (long j = (long)slot * 256 + threadIdx.x; j < N; j += stride) out[ooff + j] = j < L ? x[j] : 0.f;
        return;
    }
    // a plan that is not this call's (the tables live on the device: the kernel cannot refuse) reads nothing and writes zeros
    const bool ok = up >= 1 && down >= 1 && up <= RS_MAX_RATIO && down <= RS_MAX_RATIO && half >= 0 && base >= 0 && L >= 0 &&
                    half <= n_taps && base <= n_taps - (2 * half + 1);
    const double* h = taps + base;
    for (long j = (long)slot * 256 + threadIdx.x; j < N; j += stride) {
        double s = 0.0;
        if (ok) {
            const long c = j * down;                                      // 64-bit: beyond 2^31 for long utterances
            const long lo = c - half;
            long i0 = lo <= 0 ? 0 : (lo + up - 1) / up;                   // tap index c - i up + half <= 2 half
            long i1 = (c + half) / up;                                    // tap index >= 0
            if (i1 > L - 1) i1 = L - 1;
            long t = c + half - i0 * up;                                  // in [0, 2 half] for every i in [i0, i1]
            for (long i = i0; i <= i1; ++i, t -= up) s = fma((double)x[i], h[t], s);
        }
        float v = (float)s;
        if (quantize) v = (float)(fmin(fmax(rint(s * 32768.0), -32768.0), 32767.0) * (1.0 / 32768.0));
        out[ooff + j] = v;
    }
}

}  // namespace

extern "C" {

int mtl_resample(void* stream, const float* wav, const long* offsets, const long* out_offsets, const long* plan, const double* taps,
                 long n_taps, int K, int quantize, float* out) {
    if (!wav || !offsets || !out_offsets || !plan || !taps || !out) return MTL_EINVAL;
    if (K < 1 || K > (1 << 20) || n_taps < 1) return MTL_EINVAL;
    int slots = (RS_TARGET_GROUPS + K - 1) / K;
    slots = slots < 1 ? 1 : (slots > 256 ? 256 : slots);
    hipLaunchKernelGGL(resample_kernel, dim3(K * slots), dim3(256), 0, as_stream(stream), wav, offsets, out_offsets, plan, taps, n_taps, K,
                       slots, quantize, out);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // extern "C"
