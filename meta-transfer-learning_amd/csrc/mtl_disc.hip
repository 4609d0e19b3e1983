// Accent discriminator on the encoder output (modules/discriminator.py, trainer/asr/joint_trainer.py:29-37, utils/metrics.py:164-199):
//   pooled = sum_t enc[b, t, :],  logits = pooled . W^T + bias,  CE(logits, accent) and MSE(logits, 1/C), and their gradients down to
//   the encoder-output gradient.  Prototypes and formulas: include/mtl_hip.h "accent discriminator".
// Every sum runs in a fixed order (no atomics): two calls on the same inputs are bitwise equal.
#include "mtl_common.h"
#include "../../include/mtl_hip.h"

#define DISC_THREADS 256
#define DISC_LANES 64                       // float4 columns a workgroup covers per column pass: one 1 KiB row segment per wave
#define DISC_ROWLANES (DISC_THREADS / DISC_LANES)
#define DISC_MAX_C 64

static_assert(MTL_DISC_CHUNK % DISC_ROWLANES == 0, "row lanes split a chunk evenly");

// ---- stage 1: part[b][chunk][:] = sum of the chunk's rows of utterance b; lane = float4 column, the 4 waves take every 4th row
__global__ __launch_bounds__(DISC_THREADS) void disc_pool_partial_kernel(const float4* __restrict__ enc, int T, int d4, int chunks,
                                                                         float4* __restrict__ part) {
    __shared__ float4 s[DISC_ROWLANES][DISC_LANES];
    const int lane = threadIdx.x % DISC_LANES, rl = threadIdx.x / DISC_LANES;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int r0 = chunk * MTL_DISC_CHUNK, r1 = min(r0 + MTL_DISC_CHUNK, T);
    const float4* X = enc + (long)b * T * d4;
    for (int c0 = 0; c0 < d4; c0 += DISC_LANES) {
        const int c4 = c0 + lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < d4)
            for (int r = r0 + rl; r < r1; r += DISC_ROWLANES) {
                const float4 v = X[(long)r * d4 + c4];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        s[rl][lane] = acc;
        __syncthreads();
        if (rl == 0 && c4 < d4) {
#pragma unroll
            for (int j = 1; j < DISC_ROWLANES; ++j) {
                const float4 v = s[j][lane];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            part[((long)b * chunks + chunk) * d4 + c4] = acc;
        }
        __syncthreads();
    }
}

// ---- stage 2 + Linear: pooled[b][:] = sum of the partials in chunk order; logits[b][c] = pooled[b] . W[c] + bias[c] (wave per class)
__global__ __launch_bounds__(DISC_THREADS) void disc_pool_final_logits_kernel(const float* __restrict__ part, int chunks, int d,
                                                                              const float* __restrict__ W, const float* __restrict__ bias,
                                                                              int C, float* __restrict__ pooled, float* __restrict__ logits) {
    const int b = blockIdx.x;
    const float* p = part + (long)b * chunks * d;
    float* out = pooled + (long)b * d;
    for (int k = threadIdx.x; k < d; k += DISC_THREADS) {
        float acc = 0.f;
        for (int j = 0; j < chunks; ++j) acc += p[(long)j * d + k];
        out[k] = acc;
    }
    __syncthreads();                        // the block's own global writes are visible to it from here
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += DISC_THREADS / 64) {
        const float* w = W + (long)c * d;
        float acc = 0.f;
        for (int k = lane; k < d; k += 64) acc = fmaf(out[k], w[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) logits[(long)b * C + c] = acc + bias[c];
    }
}

// softmax statistics of one row of <= 64 logits, serially (C is small: the row is read twice from L1)
__device__ __forceinline__ void disc_row_stats(const float* __restrict__ z, int C, float& mx, float& se) {
    mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
}

// dLoss/dlogit[b][c] for loss = a CE + b MSE (the means over B and B C are part of it)
__device__ __forceinline__ float disc_dlogit(const float* __restrict__ z, int C, int c, int accent, float mx, float se, float a_B, float b_BC) {
    const float p = expf(z[c] - mx) / se;
    return a_B * (p - (c == accent ? 1.f : 0.f)) + b_BC * (z[c] - 1.f / (float)C);
}

// ---- the loss half: losses[0] = mean_b (log sum exp(z - max) - (z[accent] - max)); losses[1] = mean_{b,c} (logit - 1/C)^2 (mode 1).  One workgroup,
// thread = row (rows beyond 256 in a second turn ...), the threads' sums added in thread order.
__global__ __launch_bounds__(DISC_THREADS) void disc_loss_kernel(const float* __restrict__ logits, int B, int C, int accent, int mode,
                                                                 float* __restrict__ losses) {
    __shared__ float sce[DISC_THREADS], smse[DISC_THREADS];
    float ce = 0.f, mse = 0.f;
    const float u = 1.f / (float)C;
    for (int b = threadIdx.x; b < B; b += DISC_THREADS) {
        const float* z = logits + (long)b * C;
        float mx, se;
        disc_row_stats(z, C, mx, se);
        ce += logf(se) - (z[accent] - mx);          // no cancellation at the logits' magnitude: z[accent] - mx is exact 0 for a separated accent
        if (mode == 1) {
            float q = 0.f;
            for (int c = 0; c < C; ++c) q = fmaf(z[c] - u, z[c] - u, q);
            mse += q;
        }
    }
    sce[threadIdx.x] = ce;
    smse[threadIdx.x] = mse;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = min(B, DISC_THREADS);
        float tce = 0.f, tmse = 0.f;
        for (int i = 0; i < n; ++i) { tce += sce[i]; tmse += smse[i]; }
        losses[0] = tce / (float)B;
        if (mode == 1) losses[1] = tmse / ((float)B * (float)C);
    }
}

// dlogits[b][c] = a (softmax - onehot) / B + b 2 (logit - 1/C) / (B C)      (written: the gradient of the loss half alone)
__global__ __launch_bounds__(DISC_THREADS) void disc_loss_bwd_kernel(const float* __restrict__ logits, int B, int C, int accent, float a_B,
                                                                     float b_BC, float* __restrict__ dlogits) {
    const int b = blockIdx.x * DISC_THREADS + threadIdx.x;
    if (b >= B) return;
    const float* z = logits + (long)b * C;
    float mx, se;
    disc_row_stats(z, C, mx, se);
    for (int c = 0; c < C; ++c) dlogits[(long)b * C + c] = disc_dlogit(z, C, c, accent, mx, se, a_B, b_BC);
}

// ---- parameter gradients: workgroup (k tile, class c): dW[c][k] += sum_b dlogit[b][c] pooled[b][k] in batch order; the k tile 0
// workgroup adds dbias[c] += sum_b dlogit[b][c] as well
__global__ __launch_bounds__(DISC_THREADS) void disc_param_grad_kernel(const float* __restrict__ pooled, const float* __restrict__ logits,
                                                                       const float* __restrict__ dlogits, int accent, int B, int d, int C,
                                                                       float a_B, float b_BC, float* __restrict__ dW,
                                                                       float* __restrict__ dbias) {
    __shared__ float sdl[DISC_THREADS];
    const int c = blockIdx.y, k = blockIdx.x * DISC_THREADS + threadIdx.x;
    float acc = 0.f, accb = 0.f;
    for (int b0 = 0; b0 < B; b0 += DISC_THREADS) {
        const int nb = min(B - b0, DISC_THREADS);
        if ((int)threadIdx.x < nb && dlogits) {
            sdl[threadIdx.x] = dlogits[(long)(b0 + threadIdx.x) * C + c];
        } else if ((int)threadIdx.x < nb) {
            const float* z = logits + (long)(b0 + threadIdx.x) * C;
            float mx, se;
            disc_row_stats(z, C, mx, se);
            sdl[threadIdx.x] = disc_dlogit(z, C, c, accent, mx, se, a_B, b_BC);
        }
        __syncthreads();
        if (k < d)
            for (int i = 0; i < nb; ++i) acc = fmaf(sdl[i], pooled[(long)(b0 + i) * d + k], acc);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int i = 0; i < nb; ++i) accb += sdl[i];
        __syncthreads();
    }
    if (k < d) dW[(long)c * d + k] += acc;
    if (blockIdx.x == 0 && threadIdx.x == 0) dbias[c] += accb;
}

// ---- encoder-output gradient: workgroup (block of `rows` rows, b): denc[b][t][:] += dpool[b][:], dpool[b][k] = sum_c dlogit[b][c] W[c][k].
// One read-modify-write of denc, 16 bytes per lane.  dpool is formed once per workgroup and column pass: the four row lanes take every
// fourth class and meet in LDS in lane order, so a workgroup loads W (from L2) once; the host sizes `rows` so that these C loads per
// column stay at most a quarter of the 2 x rows accesses to denc.
__global__ __launch_bounds__(DISC_THREADS) void disc_denc_kernel(const float* __restrict__ logits, const float* __restrict__ dlogits,
                                                                 const float4* __restrict__ W, int accent, int T, int d4, int C, float a_B,
                                                                 float b_BC, int rows, float4* __restrict__ denc) {
    __shared__ float sdl[DISC_MAX_C];
    __shared__ float4 sg[DISC_ROWLANES][DISC_LANES];
    const int lane = threadIdx.x % DISC_LANES, rl = threadIdx.x / DISC_LANES;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * rows, r1 = min(r0 + rows, T);
    if ((int)threadIdx.x < C && dlogits) {
        sdl[threadIdx.x] = dlogits[(long)b * C + threadIdx.x];
    } else if ((int)threadIdx.x < C) {
        const float* z = logits + (long)b * C;
        float mx, se;
        disc_row_stats(z, C, mx, se);
        sdl[threadIdx.x] = disc_dlogit(z, C, threadIdx.x, accent, mx, se, a_B, b_BC);
    }
    __syncthreads();
    float4* D = denc + (long)b * T * d4;
    for (int c0 = 0; c0 < d4; c0 += DISC_LANES) {
        const int c4 = c0 + lane;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < d4)
            for (int c = rl; c < C; c += DISC_ROWLANES) {
                const float4 w = W[(long)c * d4 + c4];
                const float s = sdl[c];
                g.x = fmaf(s, w.x, g.x); g.y = fmaf(s, w.y, g.y); g.z = fmaf(s, w.z, g.z); g.w = fmaf(s, w.w, g.w);
            }
        sg[rl][lane] = g;
        __syncthreads();
        g = sg[0][lane];
#pragma unroll
        for (int j = 1; j < DISC_ROWLANES; ++j) {
            const float4 v = sg[j][lane];
            g.x += v.x; g.y += v.y; g.z += v.z; g.w += v.w;
        }
        if (c4 < d4)
            for (int r = r0 + rl; r < r1; r += DISC_ROWLANES) {
                float4 v = D[(long)r * d4 + c4];
                v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
                D[(long)r * d4 + c4] = v;
            }
        __syncthreads();
    }
}

// rows of one utterance per workgroup of the encoder-gradient pass: 32, more for many classes (C loads of W per 2 x rows accesses)
static inline int disc_bwd_rows(int C) { return C <= 16 ? 32 : (C <= 32 ? 64 : 128); }
static inline long disc_chunks(int T) { return ((long)T + MTL_DISC_CHUNK - 1) / MTL_DISC_CHUNK; }
static inline bool disc_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool disc_dims_ok(int B, int T, int d, int C, int accent_id, int mode) {
    return B >= 1 && B <= 65535 && T >= 1 && d >= 4 && d % 4 == 0 && C >= 1 && C <= DISC_MAX_C && accent_id >= 0 && accent_id < C &&
           (mode == 0 || mode == 1);
}

extern "C" {

long mtl_disc_workspace(int B, int T, int d) {
    if (B < 1 || T < 1 || d < 4 || d % 4 != 0) return 0;
    return (long)B * disc_chunks(T) * d * (long)sizeof(float);
}

int mtl_disc_loss_fwd(void* stream, const float* logits, int B, int C, int accent_id, int mode, float* losses) {
    if (!disc_dims_ok(B, 1, 4, C, accent_id, mode) || !logits || !losses) return MTL_EINVAL;
    hipLaunchKernelGGL(disc_loss_kernel, dim3(1), dim3(DISC_THREADS), 0, as_stream(stream), logits, B, C, accent_id, mode, losses);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_disc_loss_bwd(void* stream, const float* logits, int B, int C, int accent_id, int mode, float a, float b, float* dlogits) {
    if (!disc_dims_ok(B, 1, 4, C, accent_id, mode) || !logits || !dlogits) return MTL_EINVAL;
    const float a_B = a / (float)B, b_BC = mode == 1 ? 2.f * b / ((float)B * (float)C) : 0.f;
    hipLaunchKernelGGL(disc_loss_bwd_kernel, dim3((B + DISC_THREADS - 1) / DISC_THREADS), dim3(DISC_THREADS), 0, as_stream(stream), logits, B,
                       C, accent_id, a_B, b_BC, dlogits);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_disc_fwd(void* stream, const float* enc, int B, int T, int d, const float* W, const float* bias, int C, int accent_id, int mode,
                 float* pooled, float* logits, float* losses, float* workspace, long ws_bytes) {
    if (!disc_dims_ok(B, T, d, C, accent_id, mode) || !enc || !W || !bias || !pooled || !logits || !losses || !workspace) return MTL_EINVAL;
    if (ws_bytes < mtl_disc_workspace(B, T, d) || !disc_aligned(enc) || !disc_aligned(workspace)) return MTL_EINVAL;
    const long chunks = disc_chunks(T);
    if (chunks > 0x7fffffffL) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(disc_pool_partial_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(DISC_THREADS), 0, s,
                       reinterpret_cast<const float4*>(enc), T, d / 4, (int)chunks, reinterpret_cast<float4*>(workspace));
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(disc_pool_final_logits_kernel, dim3((unsigned)B), dim3(DISC_THREADS), 0, s, workspace, (int)chunks, d, W, bias, C,
                       pooled, logits);
    MTL_CHECK_LAUNCH();
    return mtl_disc_loss_fwd(stream, logits, B, C, accent_id, mode, losses);
}

static int disc_bwd_launch(void* stream, const float* pooled, const float* logits, const float* dlogits, const float* W, int accent_id, int B,
                           int T, int d, int C, float a_B, float b_BC, float* dW, float* dbias, float* denc) {
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(disc_param_grad_kernel, dim3((unsigned)((d + DISC_THREADS - 1) / DISC_THREADS), (unsigned)C), dim3(DISC_THREADS), 0, s,
                       pooled, logits, dlogits, accent_id, B, d, C, a_B, b_BC, dW, dbias);
    MTL_CHECK_LAUNCH();
    const int rows = disc_bwd_rows(C);
    hipLaunchKernelGGL(disc_denc_kernel, dim3((unsigned)((T + rows - 1) / rows), (unsigned)B), dim3(DISC_THREADS), 0, s, logits, dlogits,
                       reinterpret_cast<const float4*>(W), accent_id, T, d / 4, C, a_B, b_BC, rows, reinterpret_cast<float4*>(denc));
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_disc_bwd(void* stream, const float* pooled, const float* logits, const float* W, int accent_id, int B, int T, int d, int C, int mode,
                 float a, float b, float* dW, float* dbias, float* denc) {
    if (!disc_dims_ok(B, T, d, C, accent_id, mode) || !pooled || !logits || !W || !dW || !dbias || !denc) return MTL_EINVAL;
    if (!disc_aligned(W) || !disc_aligned(denc)) return MTL_EINVAL;
    const float a_B = a / (float)B, b_BC = mode == 1 ? 2.f * b / ((float)B * (float)C) : 0.f;
    return disc_bwd_launch(stream, pooled, logits, nullptr, W, accent_id, B, T, d, C, a_B, b_BC, dW, dbias, denc);
}

int mtl_disc_bwd_dlogits(void* stream, const float* pooled, const float* dlogits, const float* W, int B, int T, int d, int C, float* dW,
                         float* dbias, float* denc) {
    if (!disc_dims_ok(B, T, d, C, 0, 0) || !pooled || !dlogits || !W || !dW || !dbias || !denc) return MTL_EINVAL;
    if (!disc_aligned(W) || !disc_aligned(denc)) return MTL_EINVAL;
    return disc_bwd_launch(stream, pooled, nullptr, dlogits, W, 0, B, T, d, C, 0.f, 0.f, dW, dbias, denc);
}

}  // extern "C"
