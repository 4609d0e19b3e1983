// Batched log-mel filterbank front-end for gfx950 (MI355X): K waveforms -> the (K, 1, nfilt, Tmax) input batch of the model in two
// launches (LogFBankDataset.parse_audio, utils/data_loader.py:145-155, for every utterance of a sampled batch at once; the definition
// is the restatement in DESIGN.md section 15: parity with python_speech_features unpinned, pinned to the restatement).
//
//   launch 1 (fbank_batch_kernel): grid K * FB_SLOTS.  Workgroup (k, slot) walks the tiles slot, slot + FB_SLOTS, ... of utterance k; a
//            tile is FB_TF consecutive frames of ONE utterance for ALL nfft / 2 + 1 bins, so tile -> (utterance, first frame) is
//            arithmetic on the workgroup index and the device-resident offsets (the grid depends on K only).
//            Staging: the tile's frames are one span of (FB_TF - 1) fs + fl samples, written to LDS once as
//            p[i] = s[i] - 0.97 s[i-1], s = 32768 x (p[0] = s[0] at the utterance's start only; zeros past L).  The window is
//            rectangular and nothing is centred or reflected.
//            DFT on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32) against the fl x 2 (nfft / 2 + 1) cos / -sin table: only fl rows,
//            the zero padding to nfft costs nothing.  Roles as in mtl_spect.hip: A = basis^T (16 bins x 4 samples, from the L2-resident
//            table), B = frames (4 samples x 16 frames, from the LDS span).  A wave owns the bin blocks wave, wave + 4, ... (16 blocks of
//            16 for the bins 0 .. 255; bin 256, purely real like bin 0, rides in bin 0's imaginary slot as cos(pi n) = +-1, formed in
//            registers), real and imaginary part both, so (re^2 + im^2) / nfft is formed in registers and goes to an LDS tile
//            P[bin][frame] (row stride FB_TF + 4: the four bin rows of a store land on different banks).
//            Bands: thread (frame, band group) adds w[j][f] P[f][frame] over the band's bins in ascending order from the sparse table
//            (first bin, count, weight offset), E == 0 -> ln(2^-52) as a constant, else logf(E); stored for t < min(T_k, Tmax);
//            (sum v, sum v^2) over ALL T_k frames in fp64 per thread, reduced in a fixed order to one partial per (utterance, slot).
//            Neither a frame matrix nor a power spectrum exists in HBM.
//   launch 2 (fbank_finalize_kernel): per utterance the partials summed in slot order (fp64), mean / unbiased std over the nfilt T_k
//            values, rows normalised in place, frames [min(T_k, Tmax), Tmax) zeroed.  As in mtl_spect_batch the std is used as it
//            comes: a zero-variance utterance (digital silence throughout) is divided by zero and normalises to non-finite values,
//            which is what (v - mean) / std gives in the reference.
// No atomics: bitwise repeatable, and utterance k's rows depend on utterance k alone.
#include "mtl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FB_G = 2;                 // 16-frame column groups per tile
constexpr int FB_TF = 16 * FB_G;        // frames per tile
constexpr int FB_SLOTS = 32;            // workgroups (partials) per utterance
constexpr int FB_PSTR = FB_TF + 4;      // row stride of the power tile in floats
constexpr int FB_HEAD = 16;             // floats in front of the span: the cross-wave reduction scratch (8 doubles)
constexpr int FB_MAX_NFFT = 512;        // bounds the LDS: span <= (FB_TF - 1) 512 + 512 + 16 floats, power tile 257 rows
constexpr int FB_LDS_MAX = 112 * 1024;  // bytes: above the largest layout the checks admit (105 KB)
constexpr int FB_BG = 256 / FB_TF;      // band groups: thread (tid % FB_TF, tid / FB_TF)

// one pad word per 32: a frame stride that is a multiple of 32 words (fs = 160) would put the 16 frames of a B fragment on one bank
__device__ __forceinline__ int fb_pad(int q) { return q + (q >> 5); }

// frames of an utterance of L samples: 1 for L <= fl, else 1 + ceil((L - fl) / fs); 0 for an empty one
__device__ __forceinline__ int fb_frames(long L, int fl, int fs) {
    if (L <= 0) return 0;
    if (L <= fl) return 1;
    return 1 + (int)((L - fl + fs - 1) / fs);
}

struct FbankP {
    const float* wav;
    const long* offsets;
    const float* basis;
    const int* band;       // nfilt x 3: first bin, count, offset of the band's weights in bw
    const float* bw;
    float* out;
    double* part;
    int K, fl, fs, nfft, nbins, ldb, nfilt, n_w, Tmax;
    int lfs;               // LDS distance of two consecutive frames: min(fs, fl) (frames are packed when they do not overlap)
    int span;              // staged floats: (FB_TF - 1) lfs + fl + 16 (the last 16 are zeros: the K loop runs in trips of 16 samples)
    int poff;              // floats from the span's start to the power tile
};

__global__ __launch_bounds__(256) void fbank_batch_kernel(const FbankP p) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];
    double* red = reinterpret_cast<double*>(fb_lds);
    float* span = fb_lds + FB_HEAD;
    float* pw = span + p.poff;
    // slot-major order, as in spect_batch_kernel: the workgroups that have a tile come first and spread over the CUs
    const int k = blockIdx.x % p.K, slot = blockIdx.x / p.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, kq = lane >> 4;
    const long off = p.offsets[k];
    const long L = p.offsets[k + 1] - off;
    const int T = fb_frames(L, p.fl, p.fs);
    const int ntiles = (T + FB_TF - 1) / FB_TF;
    const int Tst = T < p.Tmax ? T : p.Tmax;
    // Bin 0 and the last bin (nfft / 2) of a real signal have no imaginary part, so the last bin's real part rides in bin 0's imaginary
    // slot: nfft / 2 bins go through the matrix cores, 16 blocks of 16 for nfft = 512 -- four per wave, none for a 257th bin alone
    const int nfblk = (p.nbins - 1 + 15) >> 4;
    const int nsteps = (p.fl + 3) >> 2;
    const float pscale = 1.f / (float)p.nfft;
    const float ln_eps = -36.04365338911715f;                             // ln(2.220446049250313e-16), rounded once
    const int tt = tid & (FB_TF - 1), jb = tid / FB_TF;
    double s = 0.0, q2 = 0.0;

    for (int tile = slot; tile < ntiles; tile += FB_SLOTS) {
        const int t0 = tile * FB_TF;
        const int nfr = T - t0 < FB_TF ? T - t0 : FB_TF;                 // frames of this tile that exist
        const int live = (nfr - 1) * p.lfs + p.fl;                        // staged positions that belong to them
        const long i0 = (long)t0 * p.fs;
        __syncthreads();                                                  // the previous tile's span and power tile have been read
        // eight sample pairs in flight per thread; the address is always a valid one (clamped), the value is zeroed afterwards
        for (int q0 = tid; q0 < p.span; q0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + 256 * u;
                long j;
                if (p.fs <= p.fl) {
                    j = i0 + q;
                } else {
                    const int fr = q / p.fl;
                    j = i0 + (long)fr * p.fs + (q - fr * p.fl);
                }
                const bool on = q < live && j < L;
                j = j < 0 ? 0 : (j >= L ? L - 1 : j);                     // L >= 1 here: an empty utterance has no tile
                const float x = p.wav[off + j];
                const float xp = p.wav[off + (j > 0 ? j - 1 : 0)];
                const float sp = j > 0 ? 32768.f * xp : 0.f;              // p[0] = s[0]: fmaf(-0.97, 0, s) is s
                v[u] = on ? fmaf(-0.97f, sp, 32768.f * x) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + 256 * u;
                if (q < p.span) span[fb_pad(q)] = v[u];
            }
        }
        __syncthreads();
        for (int fblk = wave; fblk < nfblk; fblk += 4) {                  // uniform over a wave; no barrier inside
            // A operand of this lane: bin 16 fblk + c, sample kq of every step (columns beyond nbins read as zero)
            const int fa = fblk * 16 + c;
            const bool fa_on = fa < p.nbins;
            const float* bre = p.basis + (fa_on ? fa : 0);
            const float* bim = bre + p.nbins;
            f32x4 are[FB_G], aim[FB_G];
#pragma unroll
            for (int g = 0; g < FB_G; ++g) {
                are[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                aim[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // four steps per trip, two register sets: the 8 basis values of the NEXT trip are requested before this trip's products.
            // Loads are unconditional from a clamped address and zeroed afterwards (rows beyond fl, columns beyond nbins).
            float ar[4], ai[4], br[4], bi[4];
            auto load_basis = [&](int st, float* r, float* i) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = 4 * (st + u) + kq;
                    const bool n_on = fa_on && n < p.fl;
                    const long bo = (long)(n < p.fl ? n : p.fl - 1) * p.ldb;
                    const float xr = bre[bo], xi = bim[bo];
                    r[u] = n_on ? xr : 0.f;
                    i[u] = n_on ? (fa == 0 ? ((n & 1) ? -1.f : 1.f) : xi) : 0.f;      // bin 0's slot: cos(pi n), the last bin's real part
                }
            };
            // For n >= fl the B operand below is not zero but the next frame's samples (the slack only for a tile's last frame); the
            // zeroed A operand is what cancels it.  That holds for finite waveforms, which is what a wav file gives: a non-finite
            // sample would reach the neighbouring frame's last steps as 0 * inf.
            auto products = [&](int st, const float* r, const float* i) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = 4 * (st + u) + kq;
#pragma unroll
                    for (int g = 0; g < FB_G; ++g) {
                        const float b = span[fb_pad((16 * g + c) * p.lfs + n)];   // n <= fl + 14: inside the zeroed slack
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
            // accumulator map of the 16x16 form: row (bin) 4 (lane >> 4) + register, column (frame) lane & 15
#pragma unroll
            for (int g = 0; g < FB_G; ++g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = fblk * 16 + 4 * kq + r;
                    const float re = are[g][r], im = aim[g][r];
                    if (f == 0) {
                        pw[16 * g + c] = (re * re) * pscale;
                        pw[(p.nbins - 1) * FB_PSTR + 16 * g + c] = (im * im) * pscale;
                    } else if (f < p.nbins - 1) {
                        pw[f * FB_PSTR + 16 * g + c] = (re * re + im * im) * pscale;
                    }
                }
            }
        }
        __syncthreads();
        // bands: thread (frame tt, band group jb) takes the bands jb, jb + FB_BG, ...; a band's bins in ascending order
        const int t = t0 + tt;
        for (int j = jb; j < p.nfilt; j += FB_BG) {
            int first = p.band[3 * j], cnt = p.band[3 * j + 1], wo = p.band[3 * j + 2];
            if (first < 0 || cnt < 0 || wo < 0 || first + cnt > p.nbins || wo + cnt > p.n_w) cnt = 0;   // a wrong table reads nothing
            float e = 0.f;
            for (int i = 0; i < cnt; ++i) e = fmaf(p.bw[wo + i], pw[(first + i) * FB_PSTR + tt], e);
            const float v = e == 0.f ? ln_eps : logf(e);
            if (t < T) {
                s += v;
                q2 += (double)v * v;
                if (t < Tst) p.out[((long)k * p.nfilt + j) * p.Tmax + t] = v;
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
        double* dst = p.part + ((long)k * FB_SLOTS + slot) * 2;
        dst[0] = (red[0] + red[2]) + (red[4] + red[6]);
        dst[1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

// grid (K, ceil(nfilt / 4)): a wave per band row of utterance k
__global__ __launch_bounds__(256) void fbank_finalize_kernel(float* __restrict__ out, const long* __restrict__ offsets,
                                                             const double* __restrict__ part, int fl, int fs, int nfilt, int Tmax,
                                                             int normalize) {
    __shared__ float stat[2];
    const int k = blockIdx.x;
    const int T = fb_frames(offsets[k + 1] - offsets[k], fl, fs);
    const int Tst = T < Tmax ? T : Tmax;
    if (normalize) {
        if (threadIdx.x == 0) {
            const double* src = part + (long)k * FB_SLOTS * 2;
            double s = 0.0, q = 0.0;
            for (int i = 0; i < FB_SLOTS; ++i) {
                s += src[2 * i];
                q += src[2 * i + 1];
            }
            const double n = (double)nfilt * (double)T;
            const double mean = s / n;
            const double var = (q - n * mean * mean) / (n - 1.0);
            stat[0] = (float)mean;
            stat[1] = (float)(1.0 / sqrt(var));
        }
        __syncthreads();
    }
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= nfilt) return;
    float* row = out + ((long)k * nfilt + j) * Tmax;
    if (normalize) {
        const float m = stat[0], inv = stat[1];
        for (int t = threadIdx.x & 63; t < Tst; t += 64) row[t] = (row[t] - m) * inv;
    }
    for (int t = Tst + (threadIdx.x & 63); t < Tmax; t += 64) row[t] = 0.f;
}

}  // namespace

extern "C" {

long mtl_fbank_batch_workspace(int K) {
    if (K <= 0 || K > (1 << 20)) return MTL_EINVAL;
    return (long)K * FB_SLOTS * 2 * (long)sizeof(double);               // one (sum, sum of squares) per (utterance, slot)
}

int mtl_fbank_tile_frames(void) { return FB_TF; }
int mtl_fbank_slots(void) { return FB_SLOTS; }

int mtl_fbank_batch(void* stream, const float* wav, const long* offsets, int K, int fl, int fs, int nfft, const float* basis, int ldb,
                    int nfilt, const int* band, const float* band_w, int n_w, float* out, int Tmax, int normalize, void* workspace,
                    long workspace_bytes) {
    if (!wav || !offsets || !basis || !band || !band_w || !out || !workspace) return MTL_EINVAL;
    if (K < 1 || K > (1 << 20) || fl < 1 || fl > nfft || fs < 1 || nfilt < 1 || Tmax < 1) return MTL_EINVAL;
    if (nfft < 2 || nfft > FB_MAX_NFFT || (nfft & 1) || ldb < 2 * (nfft / 2 + 1) || n_w < 1) return MTL_EINVAL;
    if (workspace_bytes < mtl_fbank_batch_workspace(K) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MTL_EINVAL;
    FbankP p = {};
    p.wav = wav, p.offsets = offsets, p.basis = basis, p.band = band, p.bw = band_w, p.out = out;
    p.part = static_cast<double*>(workspace);
    p.K = K, p.fl = fl, p.fs = fs, p.nfft = nfft, p.nbins = nfft / 2 + 1, p.ldb = ldb, p.nfilt = nfilt, p.n_w = n_w, p.Tmax = Tmax;
    p.lfs = fs < fl ? fs : fl;
    p.span = (FB_TF - 1) * p.lfs + fl + 16;
    p.poff = (p.span + (p.span >> 5) + 1 + 3) & ~3;
    const int lds = (FB_HEAD + p.poff + p.nbins * FB_PSTR) * 4;
    if (lds > FB_LDS_MAX) return MTL_EINVAL;
    static int attr = hipFuncSetAttribute(reinterpret_cast<const void*>(fbank_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          FB_LDS_MAX) == hipSuccess ? 0 : MTL_ELAUNCH;
    if (attr) return attr;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(fbank_batch_kernel, dim3(K * FB_SLOTS), dim3(256), lds, s, p);
    hipLaunchKernelGGL(fbank_finalize_kernel, dim3(K, (nfilt + 3) / 4), dim3(256), 0, s, out, offsets, p.part, fl, fs, nfilt, Tmax, normalize);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // extern "C"
