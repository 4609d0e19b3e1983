// Tempo and gain augmentation for gfx950 (MI355X) in front of the batched spectrogram front-end (load_randomly_augmented_audio,
// utils/audio.py:35-61: `sox tempo f gain g` into a 16-bit file).  What sox did is pinned by a restatement of ours (DESIGN.md section 12,
// tests/augment_util.py), parity with sox unpinned:
//
//   tempo   WSOLA.  Segment S, search R, overlap O samples, H = S - O.  Utterance k of L samples at factor f becomes N samples (the
//           out_offsets table: N = floor(L / f + 0.5) is the host's), M = ceil(N / H) segments.  Segment m starts in the input at
//           p_m = floor(f (m H) + 0.5) (fp64, one multiply and one add, never contracted: the host forms the same integer) and is
//           shifted by o_m in [0, R]: o_0 = R / 2, and for m >= 1 o_m is the c that minimises sum_{i<O} (tail_{m-1}[i] - x[p_m + c + i])^2
//           with tail_{m-1}[i] = x[p_{m-1} + o_{m-1} + H + i], the smallest c on a tie.  x reads as 0 at and beyond L.
//           Output sample j = m H + i (i < H): x[p_m + o_m + i], cross-faded over the first O samples of every segment but the first:
//           tail_{m-1}[i] + (i / O) (x[p_m + o_m + i] - tail_{m-1}[i]).  f == 1.0 bypasses the effect (no segments, a copy).
//   gain    then y = clip(rint(t g 32768), -32768, 32767) / 32768: the 16-bit file without dither.
//
//   mtl_tempo_search   one workgroup per utterance walks its segments in order (tail_m depends on o_m: the chain is inherent), a thread
//                      per candidate.  Only LDS is on the chain: the samples a link can touch do not depend on the offsets -- the
//                      candidates of segment m are x[p_m .. p_m + R + O) and every possible tail of segment m lies in
//                      x[p_m + H .. p_m + H + R + O) -- so both windows of the NEXT link are requested from memory before this link's
//                      sums are formed.  Differences and sums in fp64 in index order; arg-min over (value, index) by wave shuffles, then
//                      over the four waves in index order.
//   mtl_tempo_render   grid over (utterance, slot) like wave_mix_kernel: every output sample from seg_off, the offsets and f alone.
// No atomics: bitwise repeatable.
#include "mtl_common.h"

namespace {

constexpr int TP_SLOTS = 32;          // workgroups per utterance of the render kernel
constexpr int TP_MAXC = 256;          // candidates (R + 1) a workgroup covers, and the longest overlap
constexpr int TP_WIN = 2 * TP_MAXC;   // R + O <= 511 staged samples per window

// p_m: the same integer as the host's floor(f * (m * H) + 0.5) in IEEE fp64 (no fused multiply-add)
__device__ __forceinline__ long tp_start(double f, long m, int H) { return (long)floor(__dadd_rn(__dmul_rn(f, (double)(m * H)), 0.5)); }

// sample i of an utterance of L samples; 0 outside [0, L)
__device__ __forceinline__ float tp_x(const float* __restrict__ x, long L, long i) { return i >= 0 && i < L ? x[i] : 0.f; }

// gain and the 16-bit file as ONE expression: every path that quantises uses it
__device__ __forceinline__ float tp_gain_q(float t, float g) {
    return fminf(fmaxf(rintf(t * g * 32768.f), -32768.f), 32767.f) * (1.f / 32768.f);
}

__global__ __launch_bounds__(256) void tempo_search_kernel(const float* __restrict__ wav, const long* __restrict__ offsets,
                                                           const long* __restrict__ out_offsets, const double* __restrict__ tempo,
                                                           const long* __restrict__ seg_base, int S, int R, int O,
                                                           int* __restrict__ seg_off) {
    __shared__ double cand[TP_WIN];   // x[p_m + j], j < R + O
    __shared__ double tsup[TP_WIN];   // x[p_{m-1} + H + j], j < R + O: tail_{m-1}[i] = tsup[o_{m-1} + i]
    __shared__ double redv[4];
    __shared__ int redi[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = S - O, W = R + O;
    const long off = offsets[k];
    const long L = offsets[k + 1] - off;
    const long N = out_offsets[k + 1] - out_offsets[k];
    const long sb = seg_base[k];
    long M = (N + H - 1) / H;
    if (M > seg_base[k + 1] - sb) M = seg_base[k + 1] - sb;              // never beyond this utterance's part of the table
    const double f = tempo[k];
    if (M < 1 || f == 1.0) return;                                        // (uniform over the workgroup)
    const float* x = wav + off;
    int o_prev = R / 2;
    if (tid == 0) seg_off[sb] = o_prev;
    // windows of the next link, two samples of either per thread
    float c0, c1, t0, t1;
    auto request = [&](long m) {
        const long pc = tp_start(f, m, H), pt = tp_start(f, m - 1, H) + H;
        c0 = tp_x(x, L, pc + tid), c1 = tp_x(x, L, pc + tid + 256);
        t0 = tp_x(x, L, pt + tid), t1 = tp_x(x, L, pt + tid + 256);
    };
    if (M > 1) request(1);
    for (long m = 1; m < M; ++m) {
        __syncthreads();                                                  // the previous link's sums have been formed
        if (tid < W) cand[tid] = (double)c0, tsup[tid] = (double)t0;
        if (tid + 256 < W) cand[tid + 256] = (double)c1, tsup[tid + 256] = (double)t1;
        if (m + 1 < M) request(m + 1);                                    // in flight while this link is searched
        __syncthreads();
        double v = __builtin_huge_val();
        int idx = 0x7fffffff;
        if (tid <= R) {
            const double* tl = tsup + o_prev;                             // o_prev + O <= R + O
            double s = 0.0;
            for (int i = 0; i < O; ++i) {
                const double d = tl[i] - cand[tid + i];
                s = fma(d, d, s);                                         // (one rounding per term; exact for samples on the int16 grid)
            }
            v = s, idx = tid;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (ov < v || (ov == v && oi < idx)) v = ov, idx = oi;
        }
        if (lane == 0) redv[wave] = v, redi[wave] = idx;
        __syncthreads();
        v = redv[0], idx = redi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (redv[w] < v || (redv[w] == v && redi[w] < idx)) v = redv[w], idx = redi[w];
        o_prev = idx < 0 ? 0 : (idx > R ? R : idx);                       // (idx > R only when every sum is NaN)
        if (tid == 0) seg_off[sb + m] = o_prev;
    }
}

// grid K * TP_SLOTS: workgroup (k, slot) writes samples slot 256 + tid, + 256 TP_SLOTS, ... of the stretched utterance k
__global__ __launch_bounds__(256) void tempo_render_kernel(const float* __restrict__ wav, const long* __restrict__ offsets,
                                                           const long* __restrict__ out_offsets, const double* __restrict__ tempo,
                                                           const float* __restrict__ gain, const long* __restrict__ seg_base,
                                                           const int* __restrict__ seg_off, int K, int S, int R, int O, int quantize,
                                                           float* __restrict__ out) {
    const int k = blockIdx.x % K, slot = blockIdx.x / K;
    const int H = S - O;
    const long off = offsets[k];
    const long L = offsets[k + 1] - off;
    const long ooff = out_offsets[k];
    const long N = out_offsets[k + 1] - ooff;
    const long sb = seg_base[k], nseg = seg_base[k + 1] - sb;
    const double f = tempo[k];
    const float g = quantize ? gain[k] : 1.f;
    const float* x = wav + off;
    // a table entry outside [0, R] (a table that is not this utterance's) is clamped: the reads stay inside [0, L) whatever it holds
    auto shift = [&](long m) {
        if (m >= nseg) return 0;
        const int o = seg_off[sb + m];
        return o < 0 ? 0 : (o > R ? R : o);
    };
    for (long j = (long)slot * 256 + threadIdx.x; j < N; j += 256L * TP_SLOTS) {
        float v;
        if (f == 1.0) {
            v = tp_x(x, L, j);
        } else {
            const long m = j / H;
            const int i = (int)(j - m * H);
            v = tp_x(x, L, tp_start(f, m, H) + shift(m) + i);
            if (m >= 1 && i < O) {
                const float t = tp_x(x, L, tp_start(f, m - 1, H) + shift(m - 1) + H + i);
                v = fmaf((float)i / (float)O, v - t, t);                 // (a correctly rounded weight: three roundings in all)
            }
        }
        out[ooff + j] = quantize ? tp_gain_q(v, g) : v;
    }
}

bool tp_geometry_ok(int K, int S, int R, int O) {
    return K >= 1 && K <= (1 << 20) && O >= 1 && O <= TP_MAXC && R >= 0 && R < TP_MAXC && S > O;
}

}  // namespace

extern "C" {

int mtl_tempo_search(void* stream, const float* wav, const long* offsets, const long* out_offsets, const double* tempo, const long* seg_base,
                     int K, int seg, int search, int overlap, int* seg_off) {
    if (!wav || !offsets || !out_offsets || !tempo || !seg_base || !seg_off) return MTL_EINVAL;
    if (!tp_geometry_ok(K, seg, search, overlap)) return MTL_EINVAL;
    hipLaunchKernelGGL(tempo_search_kernel, dim3(K), dim3(256), 0, as_stream(stream), wav, offsets, out_offsets, tempo, seg_base, seg, search,
                       overlap, seg_off);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_tempo_render(void* stream, const float* wav, const long* offsets, const long* out_offsets, const double* tempo, const float* gain,
                     const long* seg_base, const int* seg_off, int K, int seg, int search, int overlap, int quantize, float* out) {
    if (!wav || !offsets || !out_offsets || !tempo || !seg_base || !seg_off || !out || (quantize && !gain)) return MTL_EINVAL;
    if (!tp_geometry_ok(K, seg, search, overlap)) return MTL_EINVAL;
    hipLaunchKernelGGL(tempo_render_kernel, dim3(K * TP_SLOTS), dim3(256), 0, as_stream(stream), wav, offsets, out_offsets, tempo, gain,
                       seg_base, seg_off, K, seg, search, overlap, quantize, out);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // extern "C"
