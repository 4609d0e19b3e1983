// The 32-channel 3 x 3 convolutions of the large_cnn front-end (reference models/asr/transformer.py: Conv 32 -> 32 + ReLU + pool,
// Conv 32 -> 64 + ReLU) on the exact split of mtl_mfma.hip ("x3"): every fp32 operand = three exact bf16 pieces, six
// v_mfma_f32_32x32x16_bf16 per block product (the piece pairs with i + j <= 2, smallest first), fp32 accumulation.  Reached through the
// x3 entry points of mtl_mfma.hip (mtl_conv3x3_*_x3[_tb]) for the shapes its 64-channel instantiations refuse.
//
// Forward / data gradient (narrow_conv_kernel).  A workgroup of four waves owns an 8 (T) x 16 (F) pixel tile and ALL output channels
// (N = 32 or 64); it is persistent over the tiles.
//   * The prepared weights of a task -- [piece][K-tile][N][32], at most 108 KiB for these shapes -- are copied into LDS once per
//     workgroup and task: the image conv_wprep_x3_kernel writes is the image the fragment reads want.
//   * Per 32-channel chunk of the reduction the 10 x 18 halo of the tile is gathered, (un-pooled,) split and stored once for all nine
//     taps as [piece][halo pixel][32] (64-byte rows, 16-byte chunks swizzled by x3_swz); a tap is a constant row offset.  The next
//     stage's halo is fetched into registers before the current stage's matrix work and committed after it.
//   * Wave w owns the tile rows 2 w, 2 w + 1: 32 pixels x N channels.  Accumulator rows are ordered (pool window, position in the
//     window), so registers 4 g .. 4 g + 3 of a lane are one 2 x 2 window in torch's scan order and the pooled epilogue needs no
//     exchange between lanes.
// Weight gradient (narrow_wgrad_kernel): the reduction runs over pixels.  The x halo is staged as above (un-swizzled) and read back
// transposed with ds_read_b64_tr_b16 (tap = row offset); a wave loads the dy fragments of its own tile rows straight from memory in
// MFMA register layout (lane = output channel, 8 pixels along F), un-pools and splits them in registers and keeps the nine 32 x 32
// tap accumulators of its output-channel block.  The waves of a workgroup add their accumulators through LDS in a fixed order and
// write one slab per workgroup; wgrad_reduce_kernel (mtl_mfma.hip) sums the slabs.
#include "mtl_conv_narrow.h"

#include "mtl_h2.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int NW_HF = 18, NW_NPIX = 10 * NW_HF;       // halo of an 8 x 16 tile
constexpr int NW_PLANE = NW_NPIX * 64;                // one piece of a 32-channel halo, bytes
constexpr int NW_NV = (NW_NPIX * 8 + 255) / 256;      // float4 per thread and halo

// x = h + m + l exactly, two values per call (the split of mtl_mfma.hip: bit-identical pieces)
__device__ __forceinline__ void split3x2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
    const float q0 = r0 - __builtin_bit_cast(float, m << 16), q1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{q0, q1}, bf16x2));
}

__device__ __forceinline__ f32x16 mfma6(const uint4 (&a)[3], const uint4 (&b)[3], f32x16 cc) {
    const bf16x8 a0 = __builtin_bit_cast(bf16x8, a[0]), a1 = __builtin_bit_cast(bf16x8, a[1]), a2 = __builtin_bit_cast(bf16x8, a[2]);
    const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]), b1 = __builtin_bit_cast(bf16x8, b[1]), b2 = __builtin_bit_cast(bf16x8, b[2]);
    cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, cc, 0, 0, 0);   // smallest terms first
    cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, cc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, cc, 0, 0, 0);
}

int device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        n = 256;
    return n;
}

template <class K>
int set_smem(K kernel, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess
               ? MTL_OK
               : MTL_ELAUNCH;
}

// ------------------------------------------------------------------ tile index space (F fastest, then T, then sample)
__device__ inline int task_rows(const NarrowConvP& p, int k) {       // tile rows of a task that has frames of its own
    const int r = ((p.widths[k] >> p.wshift) + 7) / 8;
    return r < p.ntt ? (r < 1 ? 1 : r) : p.ntt;
}

__device__ inline int total_tiles(const NarrowConvP& p) {
    if (!p.widths) return p.B * p.ntt * p.ntf;
    int total = 0;
    for (int k = 0; k < p.B / p.Bt; ++k) total += p.Bt * task_rows(p, k) * p.ntf;
    return total;
}

struct Tile {
    int b, t0, f0, task;
};
struct Cursor {       // position in the per-task index space: ids are asked for in rising order
    int k = 0, lo = 0, hi = -1, ntt = 0;
};

__device__ inline Tile tile_of(const NarrowConvP& p, int id, Cursor& c) {
    Tile t;
    int ntt = p.ntt, b0 = 0;
    if (p.widths) {
        const int per_row = p.Bt * p.ntf, nt = p.B / p.Bt;
        if (c.hi < 0 || id < c.lo) {
            c.k = 0;
            c.lo = 0;
            c.ntt = task_rows(p, 0);
            c.hi = per_row * c.ntt;
        }
        while (id >= c.hi && c.k < nt - 1) {
            ++c.k;
            c.lo = c.hi;
            c.ntt = task_rows(p, c.k);
            c.hi = c.lo + per_row * c.ntt;
        }
        id -= c.lo;
        ntt = c.ntt;
        b0 = c.k * p.Bt;
    }
    t.f0 = (id % p.ntf) * 16;
    id /= p.ntf;
    t.t0 = (id % ntt) * 8;
    t.b = b0 + id / ntt;
    t.task = t.b / p.Bt;
    return t;
}

// ------------------------------------------------------------------ halo of one 32-channel chunk: gather, (un-pool,) split, store
template <bool UNPOOL>
struct Halo {
    float4 v[NW_NV];
    uchar4 a[NW_NV];
    unsigned ok;       // bit i: element i lies inside the image; UNPOOL: bits 8 + 2 i ..: position of the source pixel in its window

    // x: (B, T, F, C) or pooled (B, Tp, Fp, C); c0: first channel of the chunk
    __device__ __forceinline__ void fetch(const float* __restrict__ x, const uint8_t* __restrict__ am, int b, int t0, int f0, int T, int F,
                                          int Tp, int Fp, int C, int c0) {
        ok = 0;
#pragma unroll
        for (int i = 0; i < NW_NV; ++i) {
            const int e = threadIdx.x + i * 256;
            const int hp = min(e >> 3, NW_NPIX - 1), c4 = (e & 7) * 4;
            const int ht = hp / NW_HF, hf = hp - ht * NW_HF;
            const int ts = t0 + ht - 1, fs = f0 + hf - 1;
            bool in = (unsigned)ts < (unsigned)T && (unsigned)fs < (unsigned)F && (e >> 3) < NW_NPIX;
            const int tc = min(max(ts, 0), T - 1), fc = min(max(fs, 0), F - 1);
            if (!UNPOOL) {
                v[i] = *reinterpret_cast<const float4*>(x + (((long)b * T + tc) * F + fc) * C + c0 + c4);
            } else {
                const int tp = tc >> 1, fp = fc >> 1;
                in = in && tp < Tp && fp < Fp;
                const long o = (((long)b * Tp + min(tp, Tp - 1)) * Fp + min(fp, Fp - 1)) * C + c0 + c4;
                v[i] = *reinterpret_cast<const float4*>(x + o);
                a[i] = *reinterpret_cast<const uchar4*>(am + o);
                ok |= (unsigned)(((fs & 1) << 1) | (ts & 1)) << (8 + 2 * i);
            }
            ok |= (in ? 1u : 0u) << i;
        }
    }
    // swz: rows swizzled by x3_swz (ds_read_b128 readers) or plain (transposing readers)
    template <bool SWZ>
    __device__ __forceinline__ void commit(unsigned char* lds) const {
#pragma unroll
        for (int i = 0; i < NW_NV; ++i) {
            const int e = threadIdx.x + i * 256;
            if ((e >> 3) >= NW_NPIX) continue;
            const int hp = e >> 3, c4 = (e & 7) * 4;
            const bool in = (ok >> i) & 1u;
            float4 w = v[i];
            if (!UNPOOL) {
                w.x = in ? w.x : 0.f, w.y = in ? w.y : 0.f, w.z = in ? w.z : 0.f, w.w = in ? w.w : 0.f;
            } else {
                const unsigned sub = (ok >> (8 + 2 * i)) & 3u;
                w.x = (in && a[i].x == sub) ? w.x : 0.f;
                w.y = (in && a[i].y == sub) ? w.y : 0.f;
                w.z = (in && a[i].z == sub) ? w.z : 0.f;
                w.w = (in && a[i].w == sub) ? w.w : 0.f;
            }
            uint2 pc[3];
            split3x2(w.x, w.y, pc[0].x, pc[1].x, pc[2].x);
            split3x2(w.z, w.w, pc[0].y, pc[1].y, pc[2].y);
            unsigned char* dst = lds + hp * 64 + (SWZ ? x3_swz(c4, hp) : c4) * 2;
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(dst + q * NW_PLANE) = pc[q];
        }
    }
};

// ------------------------------------------------------------------ forward / data gradient
template <int KC, int NB>
constexpr int conv_smem() { return 3 * 9 * KC * (32 * NB) * 64 + 3 * NW_PLANE; }

template <int KC, int NB, bool UNPOOL, int EPI>
__global__ __launch_bounds__(256) void narrow_conv_kernel(NarrowConvP p) {
    constexpr int N = 32 * NB, NKT = 9 * KC, K = 32 * KC, WBYTES = 3 * NKT * N * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char nw_lds[];
    unsigned char* wl = nw_lds;
    unsigned char* hl = nw_lds + WBYTES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, hi = lane >> 5;
    const int total = total_tiles(p);
    const int my_tiles = blockIdx.x < total ? (total - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_tiles <= 0) return;
    const int nst = my_tiles * KC;      // stages: (tile, chunk)
    Cursor cur;
    Halo<UNPOOL> halo;
    Tile nx = tile_of(p, blockIdx.x, cur);
    halo.fetch(p.x, p.am_in, nx.b, nx.t0, nx.f0, p.T, p.F, p.Tp, p.Fp, K, 0);
    // this lane's A row: pixel (2 wave + (sub & 1), 2 window + (sub >> 1)) of the tile, window = m >> 2, sub = m & 3
    const int lt = 2 * wave + (m & 1), lf = 2 * (m >> 2) + ((m >> 1) & 1);
    int cur_task = -1;
    f32x16 acc[NB];
#pragma unroll 1
    for (int st = 0; st < nst; ++st) {
        const Tile tl = nx;
        const int ch = KC == 1 ? 0 : st % KC;
        if (tl.task != cur_task) {      // (uniform; every wave is behind the barrier that ended the previous stage)
            const uint4* src = reinterpret_cast<const uint4*>(p.w3 + tl.task * p.sW);
            for (int e = threadIdx.x; e < WBYTES / 16; e += 256) reinterpret_cast<uint4*>(wl)[e] = src[e];
            cur_task = tl.task;
        }
        halo.template commit<true>(hl);
        __syncthreads();
        if (st + 1 < nst) {
            const int nch = KC == 1 ? 0 : (st + 1) % KC;
            if (nch == 0) nx = tile_of(p, blockIdx.x + ((st + 1) / KC) * gridDim.x, cur);
            halo.fetch(p.x, p.am_in, nx.b, nx.t0, nx.f0, p.T, p.F, p.Tp, p.Fp, K, nch * 32);
        }
        if (ch == 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
        }
        // data gradient: the 16 gate values of this lane's outputs are requested here, from clamped addresses, and first used behind the
        // last chunk's matrix work (one exposed memory latency per tile instead of one per output element)
        float gate[16];
        if (EPI == NARROW_DGRAD && ch == KC - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = min(tl.t0 + 2 * wave + (r & 1), p.T - 1), f = min(tl.f0 + 2 * (2 * (r >> 2) + hi) + ((r >> 1) & 1), p.F - 1);
                gate[r] = __builtin_nontemporal_load(p.act + (((long)tl.b * p.T + t) * p.F + f) * N + m);
            }
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap - kh * 3;
            const int hp = (lt + kw) * NW_HF + lf + kh;
            const unsigned char* Ar = hl + hp * 64;
            const int asw = (hp >> 2) & 3;
            const unsigned char* Br = wl + ((tap * KC + ch) * N + m) * 64;
            const int bsw = (m >> 2) & 3;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int c8 = s * 2 + hi;
                uint4 a3[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) a3[q] = *reinterpret_cast<const uint4*>(Ar + q * NW_PLANE + ((c8 ^ asw) << 4));
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    uint4 b3[3];       // (rows n and n + 32 share (n >> 2) & 3)
#pragma unroll
                    for (int q = 0; q < 3; ++q) b3[q] = *reinterpret_cast<const uint4*>(Br + (q * NKT * N + nb * 32) * 64 + ((c8 ^ bsw) << 4));
                    acc[nb] = mfma6(a3, b3, acc[nb]);
                }
            }
        }
        if (ch == KC - 1) {
            // register 4 g + j of this lane: window 2 g + hi of the wave's eight, position j (t & 1 = j & 1, f & 1 = j >> 1); column = channel m
            const float* bias = EPI == NARROW_DGRAD ? nullptr : p.bias + tl.task * p.sBias;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int col = nb * 32 + m;
                const float bb = EPI == NARROW_DGRAD ? 0.f : bias[col];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int wf = 2 * g + hi;
                    if (EPI == NARROW_POOL) {
                        const int tp = (tl.t0 >> 1) + wave, fp = (tl.f0 >> 1) + wf;
                        if (tp < p.Tp && fp < p.Fp) {
                            float best = fmaxf(acc[nb][4 * g] + bb, 0.f);
                            int idx = 0;
#pragma unroll
                            for (int j = 1; j < 4; ++j) {
                                const float xj = fmaxf(acc[nb][4 * g + j] + bb, 0.f);
                                if (xj > best) best = xj, idx = j;
                            }
                            const long o = (((long)tl.b * p.Tp + tp) * p.Fp + fp) * N + col;
                            p.y[o] = best;
                            p.am_out[o] = (uint8_t)idx;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int t = tl.t0 + 2 * wave + (j & 1), f = tl.f0 + 2 * wf + (j >> 1);
                            if (t < p.T && f < p.F) {
                                const long o = (((long)tl.b * p.T + t) * p.F + f) * N + col;
                                if (EPI == NARROW_RELU)
                                    __builtin_nontemporal_store(fmaxf(acc[nb][4 * g + j] + bb, 0.f), p.y + o);
                                else
                                    __builtin_nontemporal_store(gate[4 * g + j] > 0.f ? acc[nb][4 * g + j] : 0.f, p.y + o);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();      // the halo (and, before a task change, the weights) have been consumed
    }
}

template <int KC, int NB, bool UNPOOL, int EPI>
int launch_conv(hipStream_t s, const NarrowConvP& p) {
    constexpr int SMEM = conv_smem<KC, NB>();
    static int attr = set_smem(narrow_conv_kernel<KC, NB, UNPOOL, EPI>, SMEM);
    if (attr) return attr;
    static const int ncu = device_cus();
    const long tiles = (long)p.B * p.ntt * p.ntf;
    const int grid = (int)(tiles < ncu ? tiles : ncu);      // one workgroup per compute unit (LDS)
    hipLaunchKernelGGL((narrow_conv_kernel<KC, NB, UNPOOL, EPI>), dim3(grid), dim3(256), SMEM, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

// ------------------------------------------------------------------ weight gradient
__device__ __forceinline__ uint4 tr_read8(const unsigned char* a) {    // 8 pixels (2 x 4) of this lane's channel
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 4 * 64));
    union {
        s16x4 h[2];
        uint4 v;
    } u;
    u.h[0] = lo;
    u.h[1] = hi;
    return u.v;
}

// NCB output-channel blocks of 32; the four waves = NCB blocks x RS row groups of a tile
template <int NCB>
constexpr int wgrad_smem() {
    constexpr int red = (4 / NCB - 1) * NCB * (9 * 16 * 64 + 64) * 4;
    return red > 3 * NW_PLANE ? red : 3 * NW_PLANE;
}

template <int NCB, bool UNPOOL>
__global__ __launch_bounds__(256) void narrow_wgrad_kernel(NarrowWgradP p) {
    constexpr int RS = 4 / NCB, ROWS = 8 / RS, NB = UNPOOL ? 4 : 8, WSLAB = 9 * 16 * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char nw_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5, g = lane >> 4, x16 = lane & 15;
    const int cb = wave % NCB, rs = wave / NCB;
    const int Cout = p.Cout, T = p.T, F = p.F;
    const int wpt = gridDim.x / p.tasks, task = blockIdx.x / wpt, ls = blockIdx.x - task * wpt;      // workgroups per task, rank in the task
    if (task >= p.tasks) return;                                // (left-over workgroups: whole workgroups, before any barrier)
    const int my_tiles = ls < p.tiles ? (p.tiles - ls + wpt - 1) / wpt : 0;
    const int co = cb * 32 + l31;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    float bsum = 0.f;
    Halo<false> halo;
    float dv[ROWS][NB];
    unsigned da[ROWS], dok[ROWS];
    auto where = [&](int j, int& b, int& t0, int& f0) {
        int id = ls + j * wpt;
        f0 = (id % p.ntf) * 16;
        id /= p.ntf;
        t0 = (id % p.ntt) * 8;
        b = id / p.ntt + task * p.B;
    };
    // this lane's B fragments of the wave's rows: output channel co, pixels f0 + 8 hi .. + 7 of row t
    auto fetch_dy = [&](int b, int t0, int f0) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int t = t0 + rs * ROWS + r, fb = f0 + hi * 8;
            const bool rowok = t < p.Ty;
            da[r] = 0;
            dok[r] = 0;
            if (!UNPOOL) {
                const int tc = min(t, T - 1);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int f = fb + k;
                    dv[r][k] = p.dy[(((long)b * T + tc) * F + min(f, F - 1)) * Cout + co];
                    dok[r] |= ((rowok && f < p.Fy) ? 1u : 0u) << k;
                }
            } else {
                const int tp = min(t >> 1, p.Tp - 1), fp0 = fb >> 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int fp = fp0 + k;
                    const long o = (((long)b * p.Tp + tp) * p.Fp + min(fp, p.Fp - 1)) * Cout + co;
                    dv[r][k] = p.dy[o];
                    da[r] |= (unsigned)p.am[o] << (8 * k);
                    dok[r] |= ((rowok && fp < p.Fp) ? 1u : 0u) << k;
                }
                dok[r] |= (unsigned)(t & 1) << 8;
            }
        }
    };
    if (my_tiles > 0) {
        int b, t0, f0;
        where(0, b, t0, f0);
        halo.fetch(p.x, nullptr, b, t0, f0, T, F, 0, 0, 32, 0);
        fetch_dy(b, t0, f0);
    }
    // A fragment (transposing read): channel 16 (g & 1) + x16 of this lane, pixels 8 hi .. + 7 of a halo row: lane 4 q + r of a 16-lane
    // group addresses pixel q, channels 4 r .. 4 r + 3 of the group's block
    const int abase = (hi * 8 + (x16 >> 2)) * 64 + (16 * (g & 1) + 4 * (x16 & 3)) * 2;
#pragma unroll 1
    for (int j = 0; j < my_tiles; ++j) {
        halo.commit<false>(nw_lds);
        // the wave's dy rows of this tile: un-pool, sum (bias gradient), split -- before the registers take the next tile's
        uint4 b3[ROWS][3];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            float val[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!UNPOOL) {
                    val[k] = ((dok[r] >> k) & 1u) ? dv[r][k] : 0.f;
                } else {
                    const unsigned sub = ((unsigned)(k & 1) << 1) | ((dok[r] >> 8) & 1u);
                    val[k] = (((dok[r] >> (k >> 1)) & 1u) && ((da[r] >> (8 * (k >> 1))) & 0xffu) == sub) ? dv[r][k >> 1] : 0.f;
                }
            }
            bsum += ((val[0] + val[1]) + (val[2] + val[3])) + ((val[4] + val[5]) + (val[6] + val[7]));
            unsigned q[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) split3x2(val[2 * k], val[2 * k + 1], q[k][0], q[k][1], q[k][2]);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) b3[r][pc] = make_uint4(q[0][pc], q[1][pc], q[2][pc], q[3][pc]);
        }
        __syncthreads();
        if (j + 1 < my_tiles) {
            int b, t0, f0;
            where(j + 1, b, t0, f0);
            halo.fetch(p.x, nullptr, b, t0, f0, T, F, 0, 0, 32, 0);
            fetch_dy(b, t0, f0);
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
                const unsigned char* At = nw_lds + abase + ((rs * ROWS + r + kw) * NW_HF + kh) * 64;
                uint4 a3[3];
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) a3[pc] = tr_read8(At + pc * NW_PLANE);
                acc[tap] = mfma6(a3, b3[r], acc[tap]);
            }
        }
        __syncthreads();      // the halo has been consumed
    }
    // the row groups of an output-channel block add up in the order rs = 0, 1, ..: through LDS (free: every wave is behind the last barrier)
    float* red = reinterpret_cast<float*>(nw_lds);
    float* redb = red + (RS - 1) * NCB * WSLAB;
    bsum += __shfl_xor(bsum, 32, 64);
    if (rs > 0) {
        float* mine = red + ((rs - 1) * NCB + cb) * WSLAB;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int v = 0; v < 16; ++v) mine[(tap * 16 + v) * 64 + lane] = acc[tap][v];
        redb[((rs - 1) * NCB + cb) * 64 + lane] = bsum;
    }
    __syncthreads();
    if (rs > 0) return;
    for (int o = 0; o < RS - 1; ++o) {
        const float* other = red + (o * NCB + cb) * WSLAB;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[tap][v] += other[(tap * 16 + v) * 64 + lane];
        bsum += redb[(o * NCB + cb) * 64 + lane];
    }
    float* slab = p.partial + (long)blockIdx.x * 9 * 32 * Cout;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int ci = 8 * (v >> 2) + 4 * hi + (v & 3);
            slab[((long)tap * 32 + ci) * Cout + co] = acc[tap][v];
        }
    if (p.bias_part && hi == 0) p.bias_part[(long)blockIdx.x * Cout + co] = bsum;
}

template <int NCB, bool UNPOOL>
int launch_wgrad(hipStream_t s, const NarrowWgradP& p) {
    constexpr int SMEM = wgrad_smem<NCB>();
    static int attr = set_smem(narrow_wgrad_kernel<NCB, UNPOOL>, SMEM);
    if (attr) return attr;
    hipLaunchKernelGGL((narrow_wgrad_kernel<NCB, UNPOOL>), dim3(narrow_wgrad_slots()), dim3(256), SMEM, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // namespace

bool narrow_conv_serves(int K, int N, bool unpool, int epi) {
    if (epi == NARROW_DGRAD) return N == 32 && (K == 32 || K == 64);       // writes the 32 input channels of either layer
    return !unpool && K == 32 && (N == 32 || N == 64);
}

int narrow_conv_launch(hipStream_t s, NarrowConvP p, bool unpool, int epi) {
    if (!narrow_conv_serves(p.K, p.N, unpool, epi) || p.B < 1 || p.Bt < 1 || p.B % p.Bt) return MTL_EINVAL;
    p.ntf = (p.Fe + 15) / 16;
    p.ntt = (p.Te + 7) / 8;
    if (p.Te <= 0 || p.Fe <= 0) return MTL_OK;               // empty extent (a pooled forward with T < 2 or F < 2): no output, no launch
    if (unpool && (p.Tp < 1 || p.Fp < 1)) {                  // no pool window at all: the un-pooled gradient is zero
        return hipMemsetAsync(p.y, 0, (size_t)p.B * p.T * p.F * p.N * 4, s) == hipSuccess ? MTL_OK : MTL_ELAUNCH;
    }
    if (epi == NARROW_DGRAD) {
        if (p.K == 32) return unpool ? launch_conv<1, 1, true, NARROW_DGRAD>(s, p) : launch_conv<1, 1, false, NARROW_DGRAD>(s, p);
        return unpool ? launch_conv<2, 1, true, NARROW_DGRAD>(s, p) : launch_conv<2, 1, false, NARROW_DGRAD>(s, p);
    }
    if (epi == NARROW_POOL) return p.N == 32 ? launch_conv<1, 1, false, NARROW_POOL>(s, p) : launch_conv<1, 2, false, NARROW_POOL>(s, p);
    return p.N == 32 ? launch_conv<1, 1, false, NARROW_RELU>(s, p) : launch_conv<1, 2, false, NARROW_RELU>(s, p);
}

bool narrow_wgrad_serves(int Cin, int Cout) { return Cin == 32 && (Cout == 32 || Cout == 64); }

int narrow_wgrad_slots(void) {
    static const int ncu = device_cus();
    return ncu;
}

int narrow_wgrad_launch(hipStream_t s, NarrowWgradP p) {
    if (p.tasks < 1 || p.tasks > narrow_wgrad_slots() || p.B < 1) return MTL_EINVAL;
    p.ntf = (p.Fy + 15) / 16;
    p.ntt = (p.Ty + 7) / 8;
    p.tiles = p.ntf * p.ntt * p.B;
    if (p.Cout == 32) return p.am ? launch_wgrad<1, true>(s, p) : launch_wgrad<1, false>(s, p);
    return p.am ? launch_wgrad<2, true>(s, p) : launch_wgrad<2, false>(s, p);
}
