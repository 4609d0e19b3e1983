// SpecAugment (Park et al., 2019) for gfx950 (MI355X) BEHIND the feature launch of the batched front-end: a small time warp, a few
// frequency masks and a few time masks on the finished, normalised (K, F, Tmax) batch, in place.  No reference implementation is at
// hand: the behaviour is pinned by a definition of ours (frontend.SpecAugment, DESIGN.md section 23, tests/specaug_util.py).
//
//   table   per utterance 3 + 2 mF + 2 mT ints: tau, c, w, (f0, f) per frequency mask, (t0, t) per time mask; formed on the host
//           (SpecAugment.plan), read as uploaded.  Everything happens over columns [0, tau): the zero padding behind is never written.
//   warp    when w != c, the same map for every row: source frame c lands on output frame w, piecewise linear on either side, sampled at
//           pixel centres.  j < w: num = (2 j + 1) c - w, den = 2 w, base = 0; j >= w: num = (2 (j - w) + 1) (tau - c) - (tau - w),
//           den = 2 (tau - w), base = c.  q = floor(num / den), r = num - q den, i0 = base + q, a = (float)((double)r / (double)den),
//           clamped to the ends (a = 0 there); out[j] = x[i0] for a == 0, else fmaf(a, x[i0 + 1] - x[i0], x[i0]).
//   masks   rows [f0, f0 + f) and frames [t0, t0 + t) become +0.0f: the utterance mean of the normalised batch.
//
//   spec_augment_kernel   one workgroup per (utterance, row).  A warped row goes through LDS: [0, tau) is read once, and behind the barrier
//                         written back warped with its masks applied on the way out -- no workgroup reads what another one writes, so in
//                         place is safe.  A row that is not warped is never read: a frequency-masked row stores zeros over [0, tau), any
//                         other row its time spans, an utterance whose table asks for nothing costs no traffic at all.
//                         Row starts are (k F + r) Tmax floats, unaligned for odd Tmax: one dword per lane, a wave-instruction moves 256
//                         contiguous bytes (the full-rate shape for plain loads and stores), no wide access, no head and tail.
//                         The table lives on the device, so the kernel cannot refuse it: tau is cut to [0, Tmax], every span to the
//                         plane, and a warp is left out unless 1 <= w <= tau - 1 and 0 <= c <= tau (den > 0; i0 is clamped anyway).
//                         With tau <= 16384 every num is below 2^30 in magnitude: the integer division is 32-bit and equals the 64-bit one
//                         of the definition.
// No atomics, no workspace: bitwise repeatable.
#include "mtl_common.h"

namespace {

constexpr int SA_MAX_MASKS = 8;          // MTL_SPECAUG_MAX_MASKS of include/mtl_hip.h
constexpr int SA_MAX_FRAMES = 16384;     // MTL_SPECAUG_MAX_FRAMES: one row of fp32 in 64 KB of LDS

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// [start, start + width) cut to [0, limit) -> (lo, hi), hi <= lo for an empty span; 64-bit sum: a wrong table may hold anything
__device__ __forceinline__ void span(int start, int width, int limit, int& lo, int& hi) {
    const long e = (long)start + (long)width;
    lo = clampi(start, 0, limit);
    hi = e < 0 ? 0 : (e > limit ? limit : (int)e);
    if (width <= 0) hi = lo;
}

__global__ __launch_bounds__(256) void spec_augment_kernel(float* __restrict__ x, int F, int Tmax, const int* __restrict__ table, int mF,
                                                           int mT) {
    extern __shared__ float row[];                                        // Tmax floats
    const int k = blockIdx.x / F, r = blockIdx.x % F;
    const int* tab = table + (long)k * (3 + 2 * mF + 2 * mT);            // uniform over the workgroup: scalar loads
    const int tau = clampi(tab[0], 0, Tmax), c = tab[1], w = tab[2];
    if (tau == 0) return;
    float* xr = x + ((long)k * F + r) * Tmax;

    bool fmasked = false;
    for (int m = 0; m < mF; ++m) {
        int lo, hi;
        span(tab[3 + 2 * m], tab[4 + 2 * m], F, lo, hi);
        fmasked |= r >= lo && r < hi;
    }
    if (fmasked) {                                                        // never read: zeros over [0, tau)
        for (int j = threadIdx.x; j < tau; j += 256) xr[j] = 0.f;
        return;
    }
    int tlo[SA_MAX_MASKS], thi[SA_MAX_MASKS];
#pragma unroll
    for (int m = 0; m < SA_MAX_MASKS; ++m) {
        tlo[m] = thi[m] = 0;
        if (m < mT) span(tab[3 + 2 * mF + 2 * m], tab[4 + 2 * mF + 2 * m], tau, tlo[m], thi[m]);
    }
    const bool warp = w != c && w >= 1 && w <= tau - 1 && c >= 0 && c <= tau;
    if (!warp) {                                                          // never read: only the time spans are stored
#pragma unroll
        for (int m = 0; m < SA_MAX_MASKS; ++m)
            for (int j = tlo[m] + threadIdx.x; j < thi[m]; j += 256) xr[j] = 0.f;
        return;
    }
    for (int j = threadIdx.x; j < tau; j += 256) row[j] = xr[j];
    __syncthreads();
    for (int j = threadIdx.x; j < tau; j += 256) {
        bool masked = false;
#pragma unroll
        for (int m = 0; m < SA_MAX_MASKS; ++m) masked |= j >= tlo[m] && j < thi[m];
        float v = 0.f;
        if (!masked) {
            int num, den, base;
            if (j < w) {
                num = (2 * j + 1) * c - w, den = 2 * w, base = 0;
            } else {
                num = (2 * (j - w) + 1) * (tau - c) - (tau - w), den = 2 * (tau - w), base = c;
            }
            // floor division, den > 0, |num| < 2^30
            const int q = num >= 0 ? (int)((unsigned)num / (unsigned)den) : -(int)(((unsigned)(-num) + (unsigned)den - 1u) / (unsigned)den);
            const int rem = num - q * den;                                // in [0, den)
            int i0 = base + q;
            float a = (float)((double)rem / (double)den);
            if (i0 < 0) i0 = 0, a = 0.f;
            if (i0 >= tau - 1) i0 = tau - 1, a = 0.f;
            const float x0 = row[i0];
            v = a == 0.f ? x0 : fmaf(a, row[i0 + 1] - x0, x0);            // (a != 0 implies i0 + 1 <= tau - 1)
        }
        xr[j] = v;
    }
}

}  // namespace

extern "C" {

int mtl_spec_augment(void* stream, float* x, int K, int F, int Tmax, const int* table, int freq_masks, int time_masks) {
    if (!x || !table) return MTL_EINVAL;
    if (K < 1 || F < 1 || Tmax < 1 || Tmax > SA_MAX_FRAMES || (long)K * F > 0x7fffffffL) return MTL_EINVAL;
    if (freq_masks < 0 || freq_masks > SA_MAX_MASKS || time_masks < 0 || time_masks > SA_MAX_MASKS) return MTL_EINVAL;
    hipLaunchKernelGGL(spec_augment_kernel, dim3(K * F), dim3(256), (size_t)Tmax * sizeof(float), as_stream(stream), x, F, Tmax, table,
                       freq_masks, time_masks);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // extern "C"
