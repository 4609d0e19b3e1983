// Batched spectrogram front-end for gfx950 (MI355X): K waveforms -> the (K, 1, F, Tmax) input batch of the model in two launches
// (SpectrogramParser.parse_audio, utils/data_loader.py:65-96, for every utterance of a sampled batch at once).
//
//   launch 1 (spect_batch_kernel<G>): grid K * SP_SLOTS * (frequency blocks of 64).  Workgroup (k, slot, fb) walks the row tiles
//            slot, slot + SP_SLOTS, ... of utterance k; a row tile is 16 G consecutive frames of ONE utterance, so
//            tile -> (utterance, first frame) is arithmetic on the workgroup index and the device-resident offsets: no table and no
//            host knowledge of the lengths (the grid depends on K and F only).
//            Framing happens here: consecutive frames overlap by n_fft - hop, so the tile's frames are one contiguous span of
//            (16 G - 1) hop + n_fft samples, staged in LDS once (center=True / reflect indices resolved while staging: only an
//            utterance's first and last tiles ever see a reflected index).  No padded waveform and no frame matrix exist in HBM.
//            Product on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32) with the roles chosen for the output layout:
//            A = basis^T (16 frequencies x 4 samples, read from the L2-resident table), B = frames (4 samples x 16 frames, read
//            from the LDS span), so an accumulator holds 4 frequencies x 16 CONSECUTIVE FRAMES per lane group and the
//            (freq, time) stores are contiguous along t.  A wave owns 16 frequencies, real and imaginary columns both: the
//            magnitude is formed in registers.  v = log1p(sqrt(re^2 + im^2)) is stored for t < min(T_k, Tmax); (sum v, sum v^2) over
//            ALL T_k frames is kept in fp64 per thread over the workgroup's tiles and reduced in a fixed order to one partial per
//            (utterance, slot, frequency block).
//   launch 2 (spect_finalize_kernel): per utterance the partials summed in index order (fp64), mean / unbiased std as
//            spect_normalize_kernel (mtl_elem.hip) forms them, rows normalised in place, frames [min(T_k, Tmax), Tmax) zeroed.
// No atomics: bitwise repeatable.
//
// Noise injection (NoiseInjection.inject_noise_sample, utils/data_loader.py:383-399) rides on the staging loop: the noise corpus is one
// int16 bank resident in HBM, utterance k takes the n = L_k samples from bank[noise_off[k]] on (noise_off[k] < 0: clean), and
//   mtl_wave_mix_coef     coef[k] = level[k] sqrt(S_d / n) / sqrt(S_n / n), S_d / S_n the fp64 sums of squares of the utterance and of its
//                         noise segment: MIX_SLOTS workgroups per utterance over contiguous chunks, one fp64 partial pair each (threads
//                         stride their chunk, lanes are combined by shuffles, the four waves in index order), then one thread per
//                         utterance adds the partials in slot order.  coef = 0 for a clean utterance and for S_n = 0.
//   mtl_wave_mix          out = mix(coef[k], bank, wav): the unfused form
//   spect_batch_kernel<G, true>   stages mix(...) instead of wav: the reflect index j addresses the MIXED signal, so both reads use it
// `mix` is ONE expression (sp_mix below) in every kernel, so the fused and the unfused path agree bit for bit.
#include "mtl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SP_SLOTS = 32;          // workgroups (partials) per utterance and frequency block
constexpr int SP_FB = 64;             // frequencies per workgroup: 4 waves x 16
constexpr int SP_CAP = 24576;         // floats of LDS for the padded span (96 KB): 16 frames of n_fft = 1024 at any hop fit
constexpr int SP_HEAD = 16;           // floats in front of the span: the cross-wave reduction scratch (8 doubles)
#ifndef MTL_MIX_SLOTS
#define MTL_MIX_SLOTS 32              // workgroups per utterance of the energy pass (1: one workgroup forms the coefficient itself, one launch)
#endif
constexpr int MIX_SLOTS = MTL_MIX_SLOTS;

// one pad word per 32: a frame stride that is a multiple of 32 words (hop = 160) would put the 16 frames of a B fragment on one bank
__device__ __forceinline__ int sp_pad(int q) { return q + (q >> 5); }

struct SpectP {
    const float* wav;
    const long* offsets;
    const float* basis;
    float* out;
    double* part;
    int K, n_fft, hop, ldb, F, Tmax, nfb;
    int fs;          // LDS distance of two consecutive frames: min(hop, n_fft) (frames are packed when they do not overlap)
    int span;        // staged floats: (16 G - 1) fs + n_fft + 16 (the last 16 are zeros: the K loop runs in trips of 16 samples)
    // noise injection (spect_batch_kernel<G, true> only)
    const short* bank;
    const long* noise_off;
    const float* coef;
    long bank_len;
};

// sample i of an utterance mixed with sample i of its noise segment (utils/data_loader.py:398): fmaf(c, noise, data) in fp32 with
// noise = (float)int16 / 32768 (exact).  The bank address is clamped into [0, bank_len): a wrong table cannot read out of bounds.
// c == 0 (clean utterance, level 0, silent segment) never touches the bank and returns the sample itself, signed zeros included.
__device__ __forceinline__ float sp_mix(float c, const short* __restrict__ bank, long bank_len, long noff, long i, float x) {
    if (c == 0.f) return x;
    long b = noff + i;
    b = b < 0 ? 0 : (b >= bank_len ? bank_len - 1 : b);
    return fmaf(c, (float)bank[b] * (1.f / 32768.f), x);
}

template <int G, bool NOISE>
__global__ __launch_bounds__(256) void spect_batch_kernel(const SpectP p) {
    extern __shared__ __attribute__((aligned(16))) float sp_lds[];
    double* red = reinterpret_cast<double*>(sp_lds);
    float* span = sp_lds + SP_HEAD;
    constexpr int TF = 16 * G;
    // slot-major order: the workgroups that have a tile (low slots) are dispatched first and spread evenly over the CUs, the ones
    // without (an utterance of fewer than 32 tiles) come last and leave at once -- interleaved, they took residency slots at the
    // start and the CUs ended up with uneven numbers of working groups (measured on 16 ten-second utterances: 119 us against 67 us)
    const int k = blockIdx.x % p.K, sf = blockIdx.x / p.K, fb = sf % p.nfb, slot = sf / p.nfb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, kq = lane >> 4;
    const long off = p.offsets[k];
    const long L = p.offsets[k + 1] - off;
    const int T = L > 0 ? 1 + (int)(L / p.hop) : 0;
    const int ntiles = (T + TF - 1) / TF;
    const int Tst = T < p.Tmax ? T : p.Tmax;
    const int fbase = fb * SP_FB + wave * 16;
    const bool wave_on = fbase < p.F;
    // A operand of this lane: frequency fbase + c, sample kq of every step (columns beyond F read as zero)
    const int fa = fbase + c;
    const bool fa_on = fa < p.F;
    const float* bre = p.basis + (fa_on ? fa : 0);
    const float* bim = bre + p.F;
    const int nsteps = (p.n_fft + 3) >> 2;
    double s = 0.0, q2 = 0.0;
    float ck = 0.f;                                                       // uniform over the workgroup: 0 leaves the bank untouched
    long noff = 0;
    if constexpr (NOISE) {
        noff = p.noise_off[k];
        ck = noff < 0 ? 0.f : p.coef[k];
    }

    for (int tile = slot; tile < ntiles; tile += SP_SLOTS) {
        const int t0 = tile * TF;
        const int nfr = T - t0 < TF ? T - t0 : TF;                       // frames of this tile that exist
        const int live = (nfr - 1) * p.fs + p.n_fft;                      // staged positions that belong to them
        const long j0 = (long)t0 * p.hop - (p.n_fft >> 1);
        __syncthreads();                                                  // the previous tile's fragments have been read
        // eight loads in flight per thread (a load -> LDS store chain per element would pay a memory round trip 41 times for the
        // 10 400 samples of a 16 kHz tile): the address is always a valid one (clamped), the value is zeroed afterwards
        for (int q0 = tid; q0 < p.span; q0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + 256 * u;
                long j;
                if (p.hop <= p.n_fft) {
                    j = j0 + q;
                } else {
                    const int fr = q / p.n_fft;
                    j = j0 + (long)fr * p.hop + (q - fr * p.n_fft);
                }
                if (j < 0) j = -j;                                        // center=True, pad_mode='reflect'
                if (j >= L) j = 2 * (L - 1) - j;
                j = j < 0 ? 0 : (j >= L ? L - 1 : j);                     // a no-op for q < live when L >= n_fft / 2 + 1; never out of bounds
                float x = p.wav[off + j];
                if constexpr (NOISE) x = sp_mix(ck, p.bank, p.bank_len, noff, j, x);
                v[u] = q < live ? x : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + 256 * u;
                if (q < p.span) span[sp_pad(q)] = v[u];
            }
        }
        __syncthreads();
        if (!wave_on) continue;
        f32x4 are[G], aim[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            are[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            aim[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // four steps per trip, two register sets: the 8 basis values of the NEXT trip are requested before this trip's products (an
        // L2 round trip is longer than a trip's matrix work, and nothing else hides it inside a wave).  Loads are unconditional from a
        // clamped address and zeroed afterwards (rows beyond n_fft, columns beyond F): no divergent branch around them.
        float ar[4], ai[4], br[4], bi[4];
        auto load_basis = [&](int st, float* r, float* i) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = 4 * (st + u) + kq;
                const bool n_on = fa_on && n < p.n_fft;
                const long bo = (long)(n < p.n_fft ? n : p.n_fft - 1) * p.ldb;
                const float xr = bre[bo], xi = bim[bo];
                r[u] = n_on ? xr : 0.f;
                i[u] = n_on ? xi : 0.f;
            }
        };
        auto products = [&](int st, const float* r, const float* i) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = 4 * (st + u) + kq;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float b = span[sp_pad((16 * g + c) * p.fs + n)];    // n <= n_fft + 14: inside the zeroed slack
                    are[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(r[u], b, are[g], 0, 0, 0);
                    aim[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(i[u], b, aim[g], 0, 0, 0);
                }
            }
        };
        load_basis(0, ar, ai);
        for (int st4 = 0; st4 < nsteps; st4 += 8) {
            load_basis(st4 + 4, br, bi);
            products(st4, ar, ai);
            load_basis(st4 + 8, ar, ai);
            if (st4 + 4 < nsteps) products(st4 + 4, br, bi);
        }
        // accumulator map of the 16x16 form: row (frequency) 4 (lane >> 4) + register, column (frame) lane & 15
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int t = t0 + 16 * g + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = fbase + 4 * kq + r;
                const float re = are[g][r], im = aim[g][r];
                const float v = log1pf(sqrtf(re * re + im * im));
                if (f < p.F && t < T) {
                    s += v;
                    q2 += (double)v * v;
                    if (t < Tst) p.out[((long)k * p.F + f) * p.Tmax + t] = v;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q2 += __shfl_xor(q2, o, 64);
    }
    __syncthreads();
    if (lane == 0) {
        red[2 * wave] = s;
        red[2 * wave + 1] = q2;
    }
    __syncthreads();
    if (tid == 0) {
        double* dst = p.part + (((long)k * SP_SLOTS + slot) * p.nfb + fb) * 2;
        dst[0] = (red[0] + red[2]) + (red[4] + red[6]);
        dst[1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

// grid (K, ceil(F / 4)): a wave per frequency row of utterance k
__global__ __launch_bounds__(256) void spect_finalize_kernel(float* __restrict__ out, const long* __restrict__ offsets,
                                                             const double* __restrict__ part, int hop, int F, int Tmax, int nfb,
                                                             int normalize) {
    __shared__ float stat[2];
    const int k = blockIdx.x;
    const long L = offsets[k + 1] - offsets[k];
    const int T = L > 0 ? 1 + (int)(L / hop) : 0;
    const int Tst = T < Tmax ? T : Tmax;
    if (normalize) {
        if (threadIdx.x == 0) {
            const double* src = part + (long)k * SP_SLOTS * nfb * 2;
            double s = 0.0, q = 0.0;
            for (int i = 0; i < SP_SLOTS * nfb; ++i) {
                s += src[2 * i];
                q += src[2 * i + 1];
            }
            const double n = (double)F * (double)T;
            const double mean = s / n;
            const double var = (q - n * mean * mean) / (n - 1.0);
            stat[0] = (float)mean;
            stat[1] = (float)(1.0 / sqrt(var));
        }
        __syncthreads();
    }
    const int f = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (f >= F) return;
    float* row = out + ((long)k * F + f) * Tmax;
    if (normalize) {
        const float m = stat[0], inv = stat[1];
        for (int t = threadIdx.x & 63; t < Tst; t += 64) row[t] = (row[t] - m) * inv;
    }
    for (int t = Tst + (threadIdx.x & 63); t < Tmax; t += 64) row[t] = 0.f;
}

// energy pass: grid K * MIX_SLOTS, workgroup (k, slot) sums the squares of chunk `slot` of utterance k and of its noise segment
__global__ __launch_bounds__(256) void wave_mix_energy_kernel(const float* __restrict__ wav, const long* __restrict__ offsets, int K,
                                                              const short* __restrict__ bank, long bank_len,
                                                              const long* __restrict__ noise_off, const float* __restrict__ level,
                                                              double* __restrict__ part, float* __restrict__ coef) {
    __shared__ double red[8];
    const int k = blockIdx.x % K, slot = blockIdx.x / K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long off = offsets[k];
    const long L = offsets[k + 1] - off;
    const long noff = noise_off[k];
    const long chunk = ((L + MIX_SLOTS - 1) / MIX_SLOTS + 255) / 256 * 256;
    const long i0 = slot * chunk, i1 = i0 + chunk < L ? i0 + chunk : L;
    double sd = 0.0, sn = 0.0;
    if (noff >= 0) {
        for (long b = i0 + tid; b < i1; b += 8 * 256) {
            float d[8], n[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {                                 // eight loads of either kind in flight, from clamped addresses
                long i = b + 256 * u;
                const bool on = i < i1;
                i = on ? i : i1 - 1;
                long a = noff + i;
                a = a >= bank_len ? bank_len - 1 : a;
                d[u] = on ? wav[off + i] : 0.f;
                n[u] = on ? (float)bank[a] * (1.f / 32768.f) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sd = fma((double)d[u], (double)d[u], sd);
                sn = fma((double)n[u], (double)n[u], sn);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sd += __shfl_xor(sd, o, 64);
        sn += __shfl_xor(sn, o, 64);
    }
    if (lane == 0) {
        red[2 * wave] = sd;
        red[2 * wave + 1] = sn;
    }
    __syncthreads();
    if (tid != 0) return;
    sd = (red[0] + red[2]) + (red[4] + red[6]);
    sn = (red[1] + red[3]) + (red[5] + red[7]);
    if (MIX_SLOTS > 1) {
        part[((long)k * MIX_SLOTS + slot) * 2] = sd;
        part[((long)k * MIX_SLOTS + slot) * 2 + 1] = sn;
    } else {
        const double n = (double)L;
        coef[k] = noff >= 0 && sn > 0.0 ? (float)((double)level[k] * sqrt(sd / n) / sqrt(sn / n)) : 0.f;
    }
}

// a thread per utterance: the partials in slot order, the coefficient in fp64, rounded once to fp32
__global__ __launch_bounds__(64) void wave_mix_coef_kernel(const long* __restrict__ offsets, int K, const long* __restrict__ noise_off,
                                                           const float* __restrict__ level, const double* __restrict__ part,
                                                           float* __restrict__ coef) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    double sd = 0.0, sn = 0.0;
    for (int i = 0; i < MIX_SLOTS; ++i) {
        sd += part[((long)k * MIX_SLOTS + i) * 2];
        sn += part[((long)k * MIX_SLOTS + i) * 2 + 1];
    }
    const double n = (double)(offsets[k + 1] - offsets[k]);
    coef[k] = noise_off[k] >= 0 && sn > 0.0 ? (float)((double)level[k] * sqrt(sd / n) / sqrt(sn / n)) : 0.f;
}

// grid K * MIX_SLOTS: workgroup (k, slot) writes samples slot 256 + tid, + 256 MIX_SLOTS, ... of utterance k
__global__ __launch_bounds__(256) void wave_mix_kernel(const float* __restrict__ wav, const long* __restrict__ offsets, int K,
                                                       const short* __restrict__ bank, long bank_len, const long* __restrict__ noise_off,
                                                       const float* __restrict__ coef, float* __restrict__ out) {
    const int k = blockIdx.x % K, slot = blockIdx.x / K;
    const long off = offsets[k];
    const long L = offsets[k + 1] - off;
    const long noff = noise_off[k];
    const float ck = noff < 0 ? 0.f : coef[k];
    for (long i = (long)slot * 256 + threadIdx.x; i < L; i += 256L * MIX_SLOTS) out[off + i] = sp_mix(ck, bank, bank_len, noff, i, wav[off + i]);
}

int sp_nfb(int F) { return (F + SP_FB - 1) / SP_FB; }

template <int G, bool NOISE>
int launch_batch(hipStream_t s, const SpectP& p, int lds_bytes) {
    static int attr = hipFuncSetAttribute(reinterpret_cast<const void*>(spect_batch_kernel<G, NOISE>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (SP_HEAD + SP_CAP) * 4) == hipSuccess ? 0 : MTL_ELAUNCH;
    if (attr) return attr;
    hipLaunchKernelGGL((spect_batch_kernel<G, NOISE>), dim3(p.K * SP_SLOTS * p.nfb), dim3(256), lds_bytes, s, p);
    return MTL_OK;
}

// argument checks and the two launches shared by mtl_spect_batch and mtl_spect_batch_noise (p.bank == nullptr: the clean kernel)
template <bool NOISE>
int spect_batch(void* stream, SpectP p, int normalize, void* workspace, long workspace_bytes) {
    if (!p.wav || !p.offsets || !p.basis || !p.out || !workspace) return MTL_EINVAL;
    if (p.K < 1 || p.K > (1 << 20) || p.n_fft < 2 || p.n_fft > 1024 || (p.n_fft & 1) || p.hop < 1 || p.F != p.n_fft / 2 + 1 ||
        p.ldb < 2 * p.F || p.Tmax < 1)
        return MTL_EINVAL;
    if (workspace_bytes < (long)p.K * SP_SLOTS * sp_nfb(p.F) * 2 * (long)sizeof(double) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return MTL_EINVAL;
    p.part = static_cast<double*>(workspace);
    p.nfb = sp_nfb(p.F);
    p.fs = p.hop < p.n_fft ? p.hop : p.n_fft;
    hipStream_t s = as_stream(stream);
    int rc = MTL_EINVAL;
    for (int G = 4; G >= 1; G >>= 1) {                                   // the widest row tile whose span fits (G = 1 always does)
        p.span = (16 * G - 1) * p.fs + p.n_fft + 16;
        const int floats = p.span + (p.span >> 5) + 1;
        if (floats > SP_CAP) continue;
        const int lds = (SP_HEAD + floats) * 4;
        rc = G == 4 ? launch_batch<4, NOISE>(s, p, lds) : G == 2 ? launch_batch<2, NOISE>(s, p, lds) : launch_batch<1, NOISE>(s, p, lds);
        break;
    }
    if (rc != MTL_OK) return rc;
    hipLaunchKernelGGL(spect_finalize_kernel, dim3(p.K, (p.F + 3) / 4), dim3(256), 0, s, p.out, p.offsets, p.part, p.hop, p.F, p.Tmax, p.nfb,
                       normalize);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // namespace

extern "C" {

long mtl_spect_batch_workspace(long total_frames, int K, int F) {
    if (K <= 0 || F <= 0 || total_frames < K) return MTL_EINVAL;
    return (long)K * SP_SLOTS * sp_nfb(F) * 2 * (long)sizeof(double);   // one (sum, sum of squares) per (utterance, slot, frequency block)
}

int mtl_spect_batch(void* stream, const float* wav, const long* offsets, int K, int n_fft, int hop, const float* basis, int ldb, int F,
                    float* out, int Tmax, int normalize, void* workspace, long workspace_bytes) {
    SpectP p = {};
    p.wav = wav, p.offsets = offsets, p.basis = basis, p.out = out;
    p.K = K, p.n_fft = n_fft, p.hop = hop, p.ldb = ldb, p.F = F, p.Tmax = Tmax;
    return spect_batch<false>(stream, p, normalize, workspace, workspace_bytes);
}

long mtl_wave_mix_coef_workspace(int K) {
    if (K <= 0 || K > (1 << 20)) return MTL_EINVAL;
    return (long)K * MIX_SLOTS * 2 * (long)sizeof(double);              // one (S_d, S_n) per (utterance, slot)
}

int mtl_wave_mix_coef(void* stream, const float* wav, const long* offsets, int K, const short* bank, long bank_len, const long* noise_off,
                      const float* level, float* coef, void* workspace, long workspace_bytes) {
    if (!wav || !offsets || !bank || !noise_off || !level || !coef || !workspace) return MTL_EINVAL;
    if (K < 1 || K > (1 << 20) || bank_len <= 0) return MTL_EINVAL;
    if (workspace_bytes < mtl_wave_mix_coef_workspace(K) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(wave_mix_energy_kernel, dim3(K * MIX_SLOTS), dim3(256), 0, s, wav, offsets, K, bank, bank_len, noise_off, level, part, coef);
    if (MIX_SLOTS > 1)
        hipLaunchKernelGGL(wave_mix_coef_kernel, dim3((K + 63) / 64), dim3(64), 0, s, offsets, K, noise_off, level, part, coef);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_wave_mix(void* stream, const float* wav, const long* offsets, int K, const short* bank, long bank_len, const long* noise_off,
                 const float* coef, float* out) {
    if (!wav || !offsets || !bank || !noise_off || !coef || !out) return MTL_EINVAL;
    if (K < 1 || K > (1 << 20) || bank_len <= 0) return MTL_EINVAL;
    hipLaunchKernelGGL(wave_mix_kernel, dim3(K * MIX_SLOTS), dim3(256), 0, as_stream(stream), wav, offsets, K, bank, bank_len, noise_off, coef, out);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_spect_batch_noise(void* stream, const float* wav, const long* offsets, int K, int n_fft, int hop, const float* basis, int ldb, int F,
                          float* out, int Tmax, int normalize, void* workspace, long workspace_bytes, const short* bank, long bank_len,
                          const long* noise_off, const float* coef) {
    if (!bank || !noise_off || !coef || bank_len <= 0) return MTL_EINVAL;
    SpectP p = {};
    p.wav = wav, p.offsets = offsets, p.basis = basis, p.out = out;
    p.K = K, p.n_fft = n_fft, p.hop = hop, p.ldb = ldb, p.F = F, p.Tmax = Tmax;
    p.bank = bank, p.bank_len = bank_len, p.noise_off = noise_off, p.coef = coef;
    return spect_batch<true>(stream, p, normalize, workspace, workspace_bytes);
}

}  // extern "C"
