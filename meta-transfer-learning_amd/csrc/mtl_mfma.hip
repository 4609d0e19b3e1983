// fp32 MFMA tile engine for gfx950 (MI355X): one engine, many loaders.
//
//  * exact-f32 matrix cores: v_mfma_f32_32x32x2_f32 (157.3 TF peak; gfx950 has no TF32/xf32),
//    bitwise an fmaf chain -> meets the 1e-4 parity bar on meta-gradients without split tricks.
//  * 256-thread workgroups (4 waves, 2x2), block tiles 128x128 / 128x64 / 64x64, BK = 32,
//    double-buffered LDS with one barrier per K-tile, register-staged global->LDS copies issued
//    before the MFMA burst of the current tile (loads fly under 64..256 MFMAs).
//  * operands are staged in the orientation their HBM layout is contiguous in ("K-major" or
//    "MN-major"), so every global access is a 16-byte-per-lane coalesced load and no transposed
//    copies of activations/weights are ever materialised.
//  * the same engine runs the linears (all four transpose combinations, batched for attention),
//    the 3x3 convolutions as implicit GEMM (im2col gather in the A loader, fused bias+ReLU(+2x2
//    max-pool) epilogues, fused un-pool + ReLU-mask for the backward), and the conv weight-gradient
//    (K = pixels, split-K into a workspace + deterministic reduction).
//
// Reference ops replaced (file:line in /root/reference): nn.Linear fwd/bwd (modules/encoder.py:72,
// modules/common_layers.py:130,287-289,303, modules/decoder.py:109), torch.bmm (common_layers.py:321,329),
// nn.Conv2d/ReLU/MaxPool2d (models/asr/transformer.py:48-59).
#include <cstdlib>
#include <type_traits>

#include "mtl_common.h"
#include "mtl_h2.h"
#include "mtl_conv_narrow.h"
#include "../../include/mtl_hip.h"

namespace {

constexpr int BK = 32;
constexpr int NT = 256;

// ------------------------------------------------------------------ LDS layouts
template <int ROWS>
struct LdsK {  // element (row, k) of a [ROWS][BK] tile; stride 33 -> conflict-free ds_read_b32 across 32 rows
    static constexpr int LD = BK + 1;
    static constexpr int SIZE = ROWS * LD;
    static __device__ __forceinline__ int at(int row, int k) { return row * LD + k; }
};
template <int ROWS>
struct LdsMN {  // same tile stored [BK][ROWS+4]: 32 consecutive rows of one k are 32 consecutive banks
    static constexpr int LD = ROWS + 4;
    static constexpr int SIZE = BK * LD;
    static __device__ __forceinline__ int at(int row, int k) { return k * LD + row; }
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ------------------------------------------------------------------ plain matrix loaders
// All loaders are BRANCH-FREE: fetch() issues unconditional loads from clamped (always valid) addresses and records a
// 4-bit validity mask; the zero-fill happens in commit(), i.e. AFTER the MFMA burst of the current tile.  With bounds
// checks as branches hipcc parks an `s_waitcnt vmcnt(0)` in front of the MFMAs and the HBM latency of every K-tile is
// exposed; this way the loads stay in flight under 64..256 MFMAs.
__device__ __forceinline__ float4 mask4(float4 v, unsigned m) {
    v.x = (m & 1u) ? v.x : 0.f;
    v.y = (m & 2u) ? v.y : 0.f;
    v.z = (m & 4u) ? v.z : 0.f;
    v.w = (m & 8u) ? v.w : 0.f;
    return v;
}
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* q, unsigned m) {
    if (VEC) return *reinterpret_cast<const float4*>(q);
    // unaligned source: four dword loads, each from an in-range element
    return make_float4(q[0], q[(m & 2u) ? 1 : 0], q[(m & 4u) ? 2 : 0], q[(m & 8u) ? 3 : 0]);
}

// Source is row-major with k contiguous: tile row r, k  ->  base[(r0+r)*ld + k]
template <int ROWS, bool VEC>
struct LoadKMajor {
    using Lds = LdsK<ROWS>;
    static constexpr int NV = ROWS * BK / 4 / NT;
    struct Regs {
        float4 v[NV];
        unsigned m[NV];
    };
    const float* base;
    long ld;
    int nrows, K, kq;
    __device__ void init(const float* p, int ld_, int r0, int rows_total, int K_, int tid) {
        base = p + (long)r0 * ld_;
        ld = ld_;
        nrows = rows_total - r0;
        K = K_;
        kq = (tid & 7) * 4;
    }
    __device__ __forceinline__ void fetch(int kt, Regs& r, int tid) const {
        const int k = kt * BK + kq;
        const unsigned km = (k < K ? 1u : 0u) | (k + 1 < K ? 2u : 0u) | (k + 2 < K ? 4u : 0u) | (k + 3 < K ? 8u : 0u);
        const int kc = k < K ? k : 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int row = (tid >> 3) + i * 32;
            const bool ok = row < nrows;
            r.m[i] = ok ? km : 0u;
            r.v[i] = load4<VEC>(base + (ok ? row : 0) * ld + kc, km);
        }
    }
    __device__ __forceinline__ void commit(float* lds, const Regs& r, int tid) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float4 v = mask4(r.v[i], r.m[i]);
            const int o = Lds::at((tid >> 3) + i * 32, kq);
            lds[o] = v.x;
            lds[o + 1] = v.y;
            lds[o + 2] = v.z;
            lds[o + 3] = v.w;
        }
    }
};

// Source is row-major with the tile-row index contiguous: tile row r, k -> base[k*ld + c0 + r]
template <int ROWS, bool VEC>
struct LoadMNMajor {
    using Lds = LdsMN<ROWS>;
    static constexpr int VPR = ROWS / 4;    // float4 per k-row
    static constexpr int KPP = NT / VPR;    // k-rows per pass
    static constexpr int NV = BK / KPP;
    struct Regs {
        float4 v[NV];
        unsigned m[NV];
    };
    const float* base;
    long ld;
    int K, m4, k0;
    unsigned mm;
    __device__ void init(const float* p, int ld_, int c0, int cols_total, int K_, int tid) {
        const int ncols = cols_total - c0;
        ld = ld_;
        K = K_;
        m4 = (tid % VPR) * 4;
        k0 = tid / VPR;
        mm = (m4 < ncols ? 1u : 0u) | (m4 + 1 < ncols ? 2u : 0u) | (m4 + 2 < ncols ? 4u : 0u) | (m4 + 3 < ncols ? 8u : 0u);
        base = p + c0 + (m4 < ncols ? m4 : 0);
    }
    __device__ __forceinline__ void fetch(int kt, Regs& r, int) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int k = kt * BK + k0 + i * KPP;
            const bool ok = k < K;
            r.m[i] = ok ? mm : 0u;
            r.v[i] = load4<VEC>(base + (ok ? k : 0) * ld, mm);
        }
    }
    __device__ __forceinline__ void commit(float* lds, const Regs& r, int) const {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            *reinterpret_cast<float4*>(&lds[(k0 + i * KPP) * Lds::LD + m4]) = mask4(r.v[i], r.m[i]);
    }
};

// ------------------------------------------------------------------ the engine
template <int BM, int BN, class LA, class LB>
struct Engine {
    static constexpr int WTM = BM / 2, WTN = BN / 2;   // 2 x 2 waves
    static constexpr int TM = WTM / 32, TN = WTN / 32; // 32x32 MFMA tiles per wave
    using AL = typename LA::Lds;
    using BL = typename LB::Lds;
    static constexpr int SMEM_BYTES = 2 * (AL::SIZE + BL::SIZE) * 4;

    static __device__ __forceinline__ void zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    static __device__ __forceinline__ void run(LA& la, LB& lb, int nk, float* smem,
                                               f32x16 (&acc)[TM][TN]) {
        const int tid = threadIdx.x;
        const int lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hi = lane >> 5;
        float* As0 = smem;
        float* As1 = smem + AL::SIZE;
        float* Bs0 = smem + 2 * AL::SIZE;
        float* Bs1 = Bs0 + BL::SIZE;
        typename LA::Regs ra;
        typename LB::Regs rb;
        la.fetch(0, ra, tid);
        lb.fetch(0, rb, tid);
        la.commit(As0, ra, tid);
        lb.commit(Bs0, rb, tid);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const float* Ac = (kt & 1) ? As1 : As0;
            const float* Bc = (kt & 1) ? Bs1 : Bs0;
            const bool more = kt + 1 < nk;
            if (more) {
                la.fetch(kt + 1, ra, tid);
                lb.fetch(kt + 1, rb, tid);
            }
            // LDS -> register fragments are double-buffered across the 16 k-steps of the tile: step s+1's operands are
            // requested before step s's MFMAs issue, so a 32x32x2 MFMA group (64 cycles each) never waits on a ds_read
            float a[2][TM], b[2][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[0][i] = Ac[AL::at(wm * WTM + i * 32 + l31, hi)];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[0][j] = Bc[BL::at(wn * WTN + j * 32 + l31, hi)];
#pragma unroll
            for (int st = 0; st < BK / 2; ++st) {
                const int cur = st & 1, nxt = cur ^ 1;
                if (st + 1 < BK / 2) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[nxt][i] = Ac[AL::at(wm * WTM + i * 32 + l31, 2 * (st + 1) + hi)];
#pragma unroll
                    for (int j = 0; j < TN; ++j) b[nxt][j] = Bc[BL::at(wn * WTN + j * 32 + l31, 2 * (st + 1) + hi)];
                }
                __builtin_amdgcn_sched_barrier(0);   // pin: next step's ds_reads are issued BEFORE this step's MFMAs
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) {
                la.commit((kt & 1) ? As0 : As1, ra, tid);
                lb.commit((kt & 1) ? Bs0 : Bs1, rb, tid);
            }
            __syncthreads();
        }
    }

    // epi.store4(local_row4, local_col, v[4]): rows local_row4..+3 (4-aligned) of column local_col
    template <class Epi>
    static __device__ __forceinline__ void finish(const f32x16 (&acc)[TM][TN], const Epi& epi) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hi = lane >> 5;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float v[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    epi.store4(wm * WTM + i * 32 + 8 * g + 4 * hi, wn * WTN + j * 32 + l31, v);
                }
    }
};

// ================================================================== generic (batched) GEMM
struct GemmP {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    const float* gate;
    int M, N, K, lda, ldb, ldc, ldg;
    float alpha;
    int flags, H;
    long sAb, sAh, sBb, sBh, sCb, sCh;
    int ksplit, kchunk;   // ksplit > 1: grid.z = (batch item) * ksplit + K-chunk; raw partial tiles go to `partial`
    float* partial;       // [batch item][ksplit][M][N]
    long sBias;           // bias stride of the OUTER batch index (0: one bias for all)
    long sBiasH;          // ... and of the inner one
    int nz;               // batch items in total (grid.z without split-K)
    int Zt;               // batch items per task (third, outermost batch level); nz when there is one task
    long sAt, sBt, sCt, sBiasT;
};

// batch item z -> element offsets of its operands
struct ZOff {
    long a, b, c, bias;
};
__device__ __forceinline__ ZOff z_offsets(const GemmP& p, int z) {
    const int zt = z / p.Zt, zz = z - zt * p.Zt;
    const int zb = zz / p.H, zh = zz - zb * p.H;
    return ZOff{zt * p.sAt + zb * p.sAb + zh * p.sAh, zt * p.sBt + zb * p.sBb + zh * p.sBh, zt * p.sCt + zb * p.sCb + zh * p.sCh,
                zt * p.sBiasT + zb * p.sBias + zh * p.sBiasH};
}

struct EpiGemm {
    float* C;
    const float* bias;
    const float* gate;
    int M, N, m0, n0, ldc, ldg, flags;
    float alpha;
    __device__ __forceinline__ void store4(int lr, int lc, const float (&v)[4]) const {
        const int col = n0 + lc;
        if (col >= N) return;
        const float bb = bias ? bias[col] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = m0 + lr + j;
            if (row >= M) continue;
            float x = alpha * v[j] + bb;
            if (flags & MTL_GEMM_RELU) x = fmaxf(x, 0.f);
            if (gate) x = gate[(long)row * ldg + col] > 0.f ? x : 0.f;
            float* c = C + (long)row * ldc + col;
            if (flags & MTL_GEMM_ACCUM) x += *c;
            *c = x;
        }
    }
};

template <int BM, int BN, bool TA, bool TB, bool VEC>
__global__ __launch_bounds__(NT) void gemm_kernel(GemmP p) {
    using LA = typename std::conditional<TA, LoadMNMajor<BM, VEC>, LoadKMajor<BM, VEC>>::type;
    using LB = typename std::conditional<TB, LoadKMajor<BN, VEC>, LoadMNMajor<BN, VEC>>::type;
    using E = Engine<BM, BN, LA, LB>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int tid = threadIdx.x;
    LA la;
    LB lb;
    f32x16 acc[E::TM][E::TN];
    E::zero(acc);
    if (p.ksplit > 1) {
        // split-K: this block owns k in [k0, k0+Kc) of batch item zi; partial sums are combined in fixed order by splitk_reduce_kernel
        const int zi = blockIdx.z / p.ksplit, zs = blockIdx.z - zi * p.ksplit;
        const ZOff zo = z_offsets(p, zi);
        const int k0 = zs * p.kchunk;
        const int Kc = min(p.kchunk, p.K - k0);
        const float* A = p.A + zo.a;
        const float* B = p.B + zo.b;
        la.init(A + (TA ? (long)k0 * p.lda : (long)k0), p.lda, m0, p.M, Kc, tid);
        lb.init(B + (TB ? (long)k0 : (long)k0 * p.ldb), p.ldb, n0, p.N, Kc, tid);
        E::run(la, lb, (Kc + BK - 1) / BK, smem, acc);
        EpiGemm epi{p.partial + (long)blockIdx.z * p.M * p.N, nullptr, nullptr, p.M, p.N, m0, n0, p.N, 0, 0, 1.f};
        E::finish(acc, epi);
        return;
    }
    const ZOff zo = z_offsets(p, blockIdx.z);
    const float* A = p.A + zo.a;
    const float* B = p.B + zo.b;
    float* C = p.C + zo.c;
    la.init(A, p.lda, m0, p.M, p.K, tid);
    lb.init(B, p.ldb, n0, p.N, p.K, tid);
    E::run(la, lb, (p.K + BK - 1) / BK, smem, acc);
    const float* gate = p.gate ? p.gate + zo.c : nullptr;
    EpiGemm epi{C, p.bias ? p.bias + zo.bias : nullptr, gate, p.M, p.N, m0, n0, p.ldc, p.ldg, p.flags, p.alpha};
    E::finish(acc, epi);
}

// C = epilogue(sum_z partial[z]) -- fixed summation order, so split-K stays run-to-run deterministic
__global__ void splitk_reduce_kernel(GemmP p) {
    const long mn = (long)p.M * p.N, total = mn * p.nz;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int zi = (int)(e / mn);
        const long r = e - zi * mn;
        const int row = (int)(r / p.N), col = (int)(r - (long)row * p.N);
        const ZOff zo = z_offsets(p, zi);
        const float* part = p.partial + (long)zi * p.ksplit * mn + r;
        float s = 0.f;
        for (int z = 0; z < p.ksplit; ++z) s += part[(long)z * mn];
        float x = p.alpha * s + (p.bias ? p.bias[zo.bias + col] : 0.f);
        if (p.flags & MTL_GEMM_RELU) x = fmaxf(x, 0.f);
        const long co = zo.c;
        if (p.gate) x = p.gate[co + (long)row * p.ldg + col] > 0.f ? x : 0.f;
        float* c = p.C + co + (long)row * p.ldc + col;
        if (p.flags & MTL_GEMM_ACCUM) x += *c;
        *c = x;
    }
}

template <class K>
int set_smem(K kernel, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) ==
                   hipSuccess
               ? 0
               : MTL_ELAUNCH;
}

template <int BM, int BN, bool TA, bool TB, bool VEC>
int launch_gemm_v(const GemmP& p, int batch, hipStream_t s) {
    using LA = typename std::conditional<TA, LoadMNMajor<BM, VEC>, LoadKMajor<BM, VEC>>::type;
    using LB = typename std::conditional<TB, LoadKMajor<BN, VEC>, LoadMNMajor<BN, VEC>>::type;
    using E = Engine<BM, BN, LA, LB>;
    static int attr = set_smem(gemm_kernel<BM, BN, TA, TB, VEC>, E::SMEM_BYTES);
    if (attr) return attr;
    dim3 grid((p.N + BN - 1) / BN, (p.M + BM - 1) / BM, batch);
    hipLaunchKernelGGL((gemm_kernel<BM, BN, TA, TB, VEC>), grid, dim3(NT), E::SMEM_BYTES, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int BM, int BN, bool TA, bool TB>
int launch_gemm(const GemmP& p, int batch, hipStream_t s) {
    // 16-byte operand loads need 16-byte aligned bases/strides (true for every call of the pass except an
    // odd-width logits matrix); everything else takes the dword-load instantiation
    const bool vec = aligned16(p.A) && aligned16(p.B) && (p.lda & 3) == 0 && (p.ldb & 3) == 0 && ((p.sAb | p.sAh | p.sBb | p.sBh | p.sAt | p.sBt) & 3) == 0;
    return vec ? launch_gemm_v<BM, BN, TA, TB, true>(p, batch, s) : launch_gemm_v<BM, BN, TA, TB, false>(p, batch, s);
}

template <bool TA, bool TB>
int dispatch_gemm(GemmP& p, int batch, hipStream_t s, float* workspace, long workspace_bytes) {
    // big tiles only when they still give >= 1 workgroup per CU
    const long big = (long)((p.M + 127) / 128) * ((p.N + 127) / 128) * batch;
    if (big >= 256) return launch_gemm<128, 128, TA, TB>(p, batch, s);
    if (workspace && big >= 48 && big <= 96 && p.K >= 2048 && (batch == 1 || p.H == 1)) {
        // a long-K product with too few 128 x 128 tiles for 256 CUs (the 5120-deep input projection: 64 tiles): the big tile
        // runs 1.5x the rate of the 64 x 64 one, so split K to fill the chip (151 -> 125 us).  Measured and NOT extended to
        // 16-tile (FFN dW: 22 -> 36 us), 28-tile (69 -> 76 us) or 160-tile (128 -> 159 us) shapes.
        long S = (256 + big - 1) / big;
        if (S > p.K / 256) S = p.K / 256;
        const long fit = workspace_bytes / ((long)p.M * p.N * 4 * batch);
        if (S > fit) S = fit;
        if (S >= 2) {
            p.kchunk = (int)(((p.K + S - 1) / S + BK - 1) / BK * BK);
            p.ksplit = (p.K + p.kchunk - 1) / p.kchunk;
            p.partial = workspace;
            if (p.ksplit >= 2) {
                int rc = launch_gemm<128, 128, TA, TB>(p, batch * p.ksplit, s);
                if (rc) return rc;
                hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid_for((long)p.M * p.N * batch, 256, 1024)), dim3(256), 0, s, p);
                MTL_CHECK_LAUNCH();
                return MTL_OK;
            }
            p.ksplit = 1;
        }
    }
    const long tiles = (long)((p.M + 63) / 64) * ((p.N + 63) / 64) * batch;
    if (workspace && tiles < 192 && p.K >= 128 && (batch == 1 || p.H == 1)) {      // (b,h)-batched attention products stay unsplit
        // too few output tiles to fill 256 CUs: split K over grid.z into a workspace, then a fixed-order reduction
        long S = (512 + tiles - 1) / tiles;
        if (S > p.K / 64) S = p.K / 64;
        const long fit = workspace_bytes / ((long)p.M * p.N * 4 * batch);
        if (S > fit) S = fit;
        if (S > 32) S = 32;
        if (S >= 2) {
            p.kchunk = (int)(((p.K + S - 1) / S + BK - 1) / BK * BK);
            p.ksplit = (p.K + p.kchunk - 1) / p.kchunk;
            p.partial = workspace;
            if (p.ksplit >= 2) {
                int rc = launch_gemm<64, 64, TA, TB>(p, batch * p.ksplit, s);
                if (rc) return rc;
                hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid_for((long)p.M * p.N * batch, 256, 1024)), dim3(256), 0, s, p);
                MTL_CHECK_LAUNCH();
                return MTL_OK;
            }
            p.ksplit = 1;
        }
    }
    return launch_gemm<64, 64, TA, TB>(p, batch, s);
}

// ================================================================== 3x3 convolution, NHWC = (B, T, F, C)
// Block tile = 128 output pixels in an 8(T) x 16(F) patch x BN output channels.  Tile row m encodes
// (pool window, position in window) so that MFMA accumulator registers 4g..4g+3 of a lane are one
// 2x2 pool window: window = (m>>5)*8 + ((m>>2)&7) -> (wt = window>>3, wf = window&7);
// sub = m&3 -> t = 2*wt + (sub&1), f = 2*wf + (sub>>1)   [torch's window order: freq-major, time-minor]
struct ConvGeom {
    int B, T, F, Cin, Cout;  // dense (un-pooled) spatial extent T x F of the conv
    int Tp, Fp;              // pooled extent (T/2, F/2) when pooling / un-pooling is fused
};

__device__ __forceinline__ void tile_row_to_tf(int m, int& t, int& f) {
    const int w = (m >> 5) * 8 + ((m >> 2) & 7);
    const int sub = m & 3;
    t = 2 * (w >> 3) + (sub & 1);
    f = 2 * (w & 7) + (sub >> 1);
}

// A operand: im2col gather.  k-tile kt -> tap = kt / (C/32), channels (kt % (C/32))*32 .. +31.
// tap = kh*3 + kw reads source pixel (t + kw - 1, f + kh - 1).   UNPOOL: the source is the pooled
// gradient dp (B,Tp,Fp,C) with its 2-bit arg-max; the dense gradient is reconstructed on the fly.
template <bool UNPOOL>
struct LoadConvA {
    using Lds = LdsK<128>;
    static constexpr int NV = 4;
    struct Regs {
        float4 v[NV];
        uchar4 a[NV];
        unsigned m[NV];   // bit 0: source pixel valid; bits 1..2: position of the source pixel in its pool window
    };
    const float* x;
    const uint8_t* am;
    int T, F, C, Tp, Fp, b, kq, cch;
    int pt[NV], pf[NV];
    __device__ void init(const float* x_, const uint8_t* am_, const ConvGeom& g, int C_, int b_, int t0, int f0, int tid) {
        x = x_;
        am = am_;
        T = g.T;
        F = g.F;
        Tp = g.Tp;
        Fp = g.Fp;
        C = C_;
        b = b_;
        cch = C_ / BK;
        kq = (tid & 7) * 4;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            int t, f;
            tile_row_to_tf((tid >> 3) + i * 32, t, f);
            pt[i] = t0 + t;
            pf[i] = f0 + f;
        }
    }
    __device__ __forceinline__ void fetch(int kt, Regs& r, int) const {
        const int tap = kt / cch;
        const int c = (kt - tap * cch) * BK + kq;
        const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ts = pt[i] + kw - 1, fs = pf[i] + kh - 1;
            bool ok = (unsigned)ts < (unsigned)T && (unsigned)fs < (unsigned)F;
            const int tc = min(max(ts, 0), T - 1), fc = min(max(fs, 0), F - 1);
            if (!UNPOOL) {
                r.v[i] = *reinterpret_cast<const float4*>(x + (((long)b * T + tc) * F + fc) * C + c);
                r.m[i] = ok ? 1u : 0u;
            } else {
                const int tp = tc >> 1, fp = fc >> 1;
                ok = ok && tp < Tp && fp < Fp;
                const long o = (((long)b * Tp + min(tp, Tp - 1)) * Fp + min(fp, Fp - 1)) * C + c;
                r.a[i] = *reinterpret_cast<const uchar4*>(am + o);
                r.v[i] = *reinterpret_cast<const float4*>(x + o);
                r.m[i] = (ok ? 1u : 0u) | ((unsigned)(((fs & 1) << 1) | (ts & 1)) << 1);
            }
        }
    }
    __device__ __forceinline__ void commit(float* lds, const Regs& r, int tid) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 v = r.v[i];
            const bool ok = r.m[i] & 1u;
            if (!UNPOOL) {
                v = mask4(v, ok ? 15u : 0u);
            } else {
                const unsigned sub = r.m[i] >> 1;
                v.x = (ok && r.a[i].x == sub) ? v.x : 0.f;
                v.y = (ok && r.a[i].y == sub) ? v.y : 0.f;
                v.z = (ok && r.a[i].z == sub) ? v.z : 0.f;
                v.w = (ok && r.a[i].w == sub) ? v.w : 0.f;
            }
            const int o = Lds::at((tid >> 3) + i * 32, kq);
            lds[o] = v.x;
            lds[o + 1] = v.y;
            lds[o + 2] = v.z;
            lds[o + 3] = v.w;
        }
    }
};

typedef float f32x2v __attribute__((ext_vector_type(2)));

struct EpiConvRelu {  // y = relu(acc + bias), dense NHWC
    float* y;
    const float* bias;
    int b, t0, f0, T, F, Cout, n0;
    __device__ __forceinline__ void store4(int lr, int lc, const float (&v)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
        const float bb = bias[col];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 2 * (w >> 3) + (j & 1), f = f0 + 2 * (w & 7) + (j >> 1);
            if (t < T && f < F) __builtin_nontemporal_store(fmaxf(v[j] + bb, 0.f), y + (((long)b * T + t) * F + f) * Cout + col);
        }
    }
    // two adjacent channels lc, lc + 1 of the same four rows (the 16 x 16 x 32 consumers: a lane owns an even / odd channel pair): 8-byte stores
    __device__ __forceinline__ void store4x2(int lr, int lc, const float (&v0)[4], const float (&v1)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
        const float2 bb = *reinterpret_cast<const float2*>(bias + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 2 * (w >> 3) + (j & 1), f = f0 + 2 * (w & 7) + (j >> 1);
            const f32x2v o = {fmaxf(v0[j] + bb.x, 0.f), fmaxf(v1[j] + bb.y, 0.f)};
            if (t < T && f < F) __builtin_nontemporal_store(o, reinterpret_cast<f32x2v*>(y + (((long)b * T + t) * F + f) * Cout + col));
        }
    }
};

struct EpiConvPool {  // p = maxpool2x2(relu(acc + bias)), first-max arg index (torch tie rule)
    float* p;
    uint8_t* am;
    const float* bias;
    int b, t0, f0, Tp, Fp, Cout, n0;
    __device__ __forceinline__ void store4(int lr, int lc, const float (&v)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
        const int tp = (t0 >> 1) + (w >> 3), fp = (f0 >> 1) + (w & 7);
        if (tp >= Tp || fp >= Fp) return;
        const float bb = bias[col];
        float best = fmaxf(v[0] + bb, 0.f);
        int idx = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const float xj = fmaxf(v[j] + bb, 0.f);
            if (xj > best) {
                best = xj;
                idx = j;
            }
        }
        const long o = (((long)b * Tp + tp) * Fp + fp) * Cout + col;
        p[o] = best;
        am[o] = (uint8_t)idx;
    }
    __device__ __forceinline__ void store4x2(int lr, int lc, const float (&v0)[4], const float (&v1)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
        const int tp = (t0 >> 1) + (w >> 3), fp = (f0 >> 1) + (w & 7);
        if (tp >= Tp || fp >= Fp) return;
        const float2 bb = *reinterpret_cast<const float2*>(bias + col);
        float best0 = fmaxf(v0[0] + bb.x, 0.f), best1 = fmaxf(v1[0] + bb.y, 0.f);
        int idx0 = 0, idx1 = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const float x0 = fmaxf(v0[j] + bb.x, 0.f), x1 = fmaxf(v1[j] + bb.y, 0.f);
            if (x0 > best0) best0 = x0, idx0 = j;
            if (x1 > best1) best1 = x1, idx1 = j;
        }
        const long o = (((long)b * Tp + tp) * Fp + fp) * Cout + col;
        *reinterpret_cast<float2*>(p + o) = make_float2(best0, best1);
        *reinterpret_cast<unsigned short*>(am + o) = (unsigned short)(idx0 | (idx1 << 8));
    }
};

struct EpiConvDgrad {  // dx = acc masked by the ReLU of the forward activation at the same place
    float* dx;
    const float* act;
    int b, t0, f0, T, F, Cout, n0;
    __device__ __forceinline__ void store4(int lr, int lc, const float (&v)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 2 * (w >> 3) + (j & 1), f = f0 + 2 * (w & 7) + (j >> 1);
            if (t < T && f < F) {
                const long o = (((long)b * T + t) * F + f) * Cout + col;
                dx[o] = act[o] > 0.f ? v[j] : 0.f;
            }
        }
    }
    // two-phase form for epilogues that own many accumulator groups: gate4 for a batch of groups first (all loads in flight
    // together), then store4g -- one exposed HBM latency per batch instead of one per group
    __device__ __forceinline__ void gate4(int lr, int lc, float (&m)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) {        // unconditional loads from clamped addresses: no branch between the loads
            const int t = min(t0 + 2 * (w >> 3) + (j & 1), T - 1), f = min(f0 + 2 * (w & 7) + (j >> 1), F - 1);
            m[j] = __builtin_nontemporal_load(act + (((long)b * T + t) * F + f) * Cout + col);
        }
    }
    __device__ __forceinline__ void store4g(int lr, int lc, const float (&v)[4], const float (&m)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 2 * (w >> 3) + (j & 1), f = f0 + 2 * (w & 7) + (j >> 1);
            if (t < T && f < F) __builtin_nontemporal_store(m[j] > 0.f ? v[j] : 0.f, dx + (((long)b * T + t) * F + f) * Cout + col);
        }
    }
    __device__ __forceinline__ void gate4x2(int lr, int lc, f32x2v (&m)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = min(t0 + 2 * (w >> 3) + (j & 1), T - 1), f = min(f0 + 2 * (w & 7) + (j >> 1), F - 1);
            m[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x2v*>(act + (((long)b * T + t) * F + f) * Cout + col));
        }
    }
    __device__ __forceinline__ void store4x2g(int lr, int lc, const float (&v0)[4], const float (&v1)[4], const f32x2v (&m)[4]) const {
        const int col = n0 + lc;
        const int w = (lr >> 5) * 8 + ((lr >> 2) & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 2 * (w >> 3) + (j & 1), f = f0 + 2 * (w & 7) + (j >> 1);
            const f32x2v o = {m[j].x > 0.f ? v0[j] : 0.f, m[j].y > 0.f ? v1[j] : 0.f};
            if (t < T && f < F) __builtin_nontemporal_store(o, reinterpret_cast<f32x2v*>(dx + (((long)b * T + t) * F + f) * Cout + col));
        }
    }
};

struct ConvP {
    const float* x;      // A source: activations (B,T,F,Cin) or pooled gradient (B,Tp,Fp,Cin) when UNPOOL
    const uint8_t* am_in;
    const float* w;      // [9][Cin][Cout], already in the tap order the A loader walks
    const float* bias;
    const float* act;    // dgrad: forward activation whose ReLU gates the output
    float* y;
    uint8_t* am_out;
    ConvGeom g;
    int ntile;           // Cout / BN
};

enum { EPI_RELU = 0, EPI_POOL = 1, EPI_DGRAD = 2 };

template <int BN, bool UNPOOL, int EPI>
__global__ __launch_bounds__(NT) void conv3x3_kernel(ConvP p) {
    using LA = LoadConvA<UNPOOL>;
    using LB = LoadMNMajor<BN, true>;
    using E = Engine<128, BN, LA, LB>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.z / p.ntile, n0 = (blockIdx.z % p.ntile) * BN;
    const int t0 = blockIdx.y * 8, f0 = blockIdx.x * 16;
    LA la;
    LB lb;
    la.init(p.x, p.am_in, p.g, p.g.Cin, b, t0, f0, tid);
    lb.init(p.w, p.g.Cout, n0, p.g.Cout, 9 * p.g.Cin, tid);
    f32x16 acc[E::TM][E::TN];
    E::zero(acc);
    E::run(la, lb, 9 * p.g.Cin / BK, smem, acc);
    if (EPI == EPI_RELU) {
        EpiConvRelu e{p.y, p.bias, b, t0, f0, p.g.T, p.g.F, p.g.Cout, n0};
        E::finish(acc, e);
    } else if (EPI == EPI_POOL) {
        EpiConvPool e{p.y, p.am_out, p.bias, b, t0, f0, p.g.Tp, p.g.Fp, p.g.Cout, n0};
        E::finish(acc, e);
    } else {
        EpiConvDgrad e{p.y, p.act, b, t0, f0, p.g.T, p.g.F, p.g.Cout, n0};
        E::finish(acc, e);
    }
}

template <int BN, bool UNPOOL, int EPI>
int launch_conv(const ConvP& p, int Te, int Fe, hipStream_t s) {
    using E = Engine<128, BN, LoadConvA<UNPOOL>, LoadMNMajor<BN, true>>;
    static int attr = set_smem(conv3x3_kernel<BN, UNPOOL, EPI>, E::SMEM_BYTES);
    if (attr) return attr;
    dim3 grid((Fe + 15) / 16, (Te + 7) / 8, p.g.B * p.ntile);
    hipLaunchKernelGGL((conv3x3_kernel<BN, UNPOOL, EPI>), grid, dim3(NT), E::SMEM_BYTES, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

template <bool UNPOOL, int EPI>
int dispatch_conv(ConvP& p, int Te, int Fe, hipStream_t s) {
    if (p.g.Cin % 32 || p.g.Cout % 64) return MTL_EINVAL;
    if (p.g.Cout % 128 == 0) {
        p.ntile = p.g.Cout / 128;
        return launch_conv<128, UNPOOL, EPI>(p, Te, Fe, s);
    }
    p.ntile = p.g.Cout / 64;
    return launch_conv<64, UNPOOL, EPI>(p, Te, Fe, s);
}

// ------------------------------------------------------------------ split-bf16 ("x3") convolution: fp32-exact results at the bf16 MFMA rate
// Every fp32 operand is split EXACTLY into three bf16 pieces (x = h + m + l: 3 x 8 significand bits); a product is the sum
// of the six piece products with i+j <= 4 (the dropped ones are < 2^-24 relative), accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16.  Six bf16 MFMAs of K=16 (32 cycles each) replace eight fp32 MFMAs of K=2 (64 cycles each):
// 2.67x the fp32 matrix roof with fp32-class error (CPU emulation: 4.7e-7 rms vs 3.2e-7 for an fp32 GEMM, K = 1152).
// Same tile geometry / epilogues as conv3x3_kernel; LDS holds three bf16 planes per operand, K-contiguous rows of
// 32 bf16 padded to 80 B (ds_read_b128 fragment reads hit 16 distinct 16-B slots), single-buffered, 2 workgroups per CU.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int X3_ROWB = 80;                      // bytes per LDS row

__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// The same split for two values at once: v_cvt_pk_bf16_f32 converts a pair per instruction and the residuals become
// v_pk_add_f32 (20 VALU per float4 instead of 36 with the scalar form; bit-identical pieces).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3x2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
    const float q0 = r0 - __builtin_bit_cast(float, m << 16), q1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{q0, q1}, bf16x2));
}
__device__ __forceinline__ void split3x4(const float4& v, bf16x4& h, bf16x4& m, bf16x4& l) {
    uint2 hh, mm, ll;
    split3x2(v.x, v.y, hh.x, mm.x, ll.x);
    split3x2(v.z, v.w, hh.y, mm.y, ll.y);
    h = __builtin_bit_cast(bf16x4, hh);
    m = __builtin_bit_cast(bf16x4, mm);
    l = __builtin_bit_cast(bf16x4, ll);
}

// two fp16 pieces ("h2"): mtl_h2.h
// NP 16-bit pieces per fp32 value: 3 = exact bf16 triple (scale ignored), 2 = fp16 pair of the scaled value
typedef float f32x4 __attribute__((ext_vector_type(4)));
#ifndef X3H_IH
#define X3H_IH 0           // probe builds: row blocks (of 16 pixels) per A-fragment batch of the 16 x 16 x 32 consumers (default 2)
#endif
#ifndef X3H_M16
#define X3H_M16 1          // consumers of conv3x3_x3h_kernel on 16 x 16 x 32 matrix instructions (0: 32 x 32 x 16, A/B builds)
#endif
// routes of the two-piece fp16 data gradients with 64 output channels (A/B builds; 0 = the 32-channel consumer waves, WN = 2, of before)
#ifndef X3H_DG2
#define X3H_DG2 1          // un-pooling source, 64 reduction channels (conv2): 1 = 16 x 16 tiles, four consumer waves of 64 px x 64 ch
#endif
#ifndef X3H_DG5
#define X3H_DG5 1          // dense source, 128 reduction channels (conv5): 64 px x 64 ch waves on 1 = 32 x 32 x 16, 2 = 16 x 16 x 32 instructions
#endif                     // (2 is 6 % faster than 1, but sums in another order than the 32 x 32 x 16 kernel it replaces: last-bit differences)
template <int NP>
struct Split;
template <>
struct Split<3> {
    static __device__ __forceinline__ void x2(float x0, float x1, float, unsigned (&pc)[3]) { split3x2(x0, x1, pc[0], pc[1], pc[2]); }
    static __device__ __forceinline__ f32x16 mfma(const uint4 (&a)[3], const uint4 (&b)[3], f32x16 cc) {
        const bf16x8 a0 = __builtin_bit_cast(bf16x8, a[0]), a1 = __builtin_bit_cast(bf16x8, a[1]), a2 = __builtin_bit_cast(bf16x8, a[2]);
        const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]), b1 = __builtin_bit_cast(bf16x8, b[1]), b2 = __builtin_bit_cast(bf16x8, b[2]);
        cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, cc, 0, 0, 0);   // smallest terms first
        cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, cc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, cc, 0, 0, 0);
    }
    // the same product on 16 x 16 x 32 instructions (one 16-byte fragment per lane covers all 32 k of the chunk)
    static __device__ __forceinline__ f32x4 mfma16(const uint4 (&a)[3], const uint4 (&b)[3], f32x4 cc) {
        const bf16x8 a0 = __builtin_bit_cast(bf16x8, a[0]), a1 = __builtin_bit_cast(bf16x8, a[1]), a2 = __builtin_bit_cast(bf16x8, a[2]);
        const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]), b1 = __builtin_bit_cast(bf16x8, b[1]), b2 = __builtin_bit_cast(bf16x8, b[2]);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, cc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, cc, 0, 0, 0);
    }
};
template <>
struct Split<2> {
    static __device__ __forceinline__ void x2(float x0, float x1, float s, unsigned (&pc)[2]) { split2x2(x0 * s, x1 * s, pc[0], pc[1]); }
    static __device__ __forceinline__ f32x16 mfma(const uint4 (&a)[2], const uint4 (&b)[2], f32x16 cc) { return h2_mfma(a, b, cc); }
    static __device__ __forceinline__ f32x4 mfma16(const uint4 (&a)[2], const uint4 (&b)[2], f32x4 cc) {
        const f16x8 a0 = __builtin_bit_cast(f16x8, a[0]), a1 = __builtin_bit_cast(f16x8, a[1]);
        const f16x8 b0 = __builtin_bit_cast(f16x8, b[0]), b1 = __builtin_bit_cast(f16x8, b[1]);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b0, cc, 0, 0, 0);           // smallest terms first
        cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b1, cc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, cc, 0, 0, 0);
    }
};
template <int NP>
__device__ __forceinline__ void split_x4(const float4& v, float s, uint2 (&pc)[NP]) {
    unsigned a[NP], b[NP];
    Split<NP>::x2(v.x, v.y, s, a);
    Split<NP>::x2(v.z, v.w, s, b);
#pragma unroll
    for (int q = 0; q < NP; ++q) pc[q] = make_uint2(a[q], b[q]);
}

// (Cout,Cin,3,3) fp32 -> bf16 pieces laid out per K-TILE: w3f[piece][kt = tap*Cin/32 + cin/32][cout][cin%32] and
// w3d[piece][kt = (8-tap)*Cout/32 + cout/32][cin][cout%32]: the rows a workgroup stages for one K-tile are one contiguous
// block of full cache lines, which is exactly the LDS image the convolution wants, so it is moved by global_load_lds
// (lane-linear destination) without touching a register.  Rows are 64 bytes = four 16-byte chunks (8 k-values each);
// chunk c of row r is stored at position c ^ ((r >> 2) & 3), which makes the consumers' ds_read_b128 of one chunk from
// 16 rows {0-3,12-15,20-27} conflict-free with no padding.

// NP = 2: the planes are followed by one fp32 -- the power-of-two scale the pieces were taken at (conv_wscale_kernel).
constexpr int WSCALE_PARTS = 16;
template <int NP>
__global__ void conv_wprep_x3_kernel(const float* w, unsigned short* wf, unsigned short* wd, int Cout, int Cin) {
    const int total = 9 * Cin * Cout;
    const int nkf = 9 * (Cin / 32), nkd = 9 * (Cout / 32);
    float s = 1.f;
    if (NP == 2) {      // trailer: [scale][16 partial maxima from conv_wscale_kernel] for both buffers
        float* hf = reinterpret_cast<float*>(wf + (long)NP * total);
        float mx = 0.f;
#pragma unroll
        for (int i = 1; i <= WSCALE_PARTS; ++i) mx = fmaxf(mx, hf[i]);
        s = pow2_scale(mx);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            hf[0] = s;
            *reinterpret_cast<float*>(wd + (long)NP * total) = s;
        }
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int tap = e % 9;
        const int cin = (e / 9) % Cin;
        const int cout = e / (9 * Cin);
        unsigned pc[NP];
        Split<NP>::x2(w[e], 0.f, s, pc);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned short v = (unsigned short)(pc[p] & 0xffffu);
            wf[(((long)p * nkf + tap * (Cin / 32) + (cin >> 5)) * Cout + cout) * 32 + x3_swz(cin & 31, cout)] = v;
            wd[(((long)p * nkd + (8 - tap) * (Cout / 32) + (cout >> 5)) * Cin + cin) * 32 + x3_swz(cout & 31, cin)] = v;
        }
    }
}

// WSCALE_PARTS workgroups: max|w| of one slice each into trailer[1 + part] of the forward buffer (plain stores: no atomics, no
// reset; one workgroup took 13 us for 147 k weights)
__global__ __launch_bounds__(256) void conv_wscale_kernel(const float* w, int total, float* hdr_f) {
    __shared__ float sh[4];
    float mx = 0.f;
    for (int e = (blockIdx.x * 256 + threadIdx.x) * 4; e < total; e += WSCALE_PARTS * 1024) {
        const float4 v = *reinterpret_cast<const float4*>(w + e);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) hdr_f[1 + blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

struct ConvX3P {
    const float* x;
    const uint8_t* am_in;
    const unsigned char* w3;   // [NP][K-tile][N rows = output channels][32] 16-bit pieces (+ fp32 scale when NP = 2): conv_wprep_x3_kernel
    const float* bias;
    const float* act;
    float* y;
    uint8_t* am_out;
    ConvGeom g;          // Cin = reduction channels, Cout = output channels of THIS conv (dgrad: swapped by the caller)
    int ntile;
    int dbg;             // ablation switches of probe builds, 0 in production
    int ntf, ntt, tiles; // halo kernel: pixel tiles along F and T, and tiles in total (F fastest, then T, then output-channel tile, then sample)
    const float* amax_in;   // NP = 2: MTL_AMAX_SLOTS floats whose maximum is >= max|x|
    float* amax_out;        // optional: atomic max of an upper bound of max|y| (the next layer's amax_in)
    // several tasks in ONE launch (round 5: the samples of task k are b in [k Bt, (k + 1) Bt); g.B counts all of them): task k reads its
    // prepared weights at w3 + k sW bytes, its bias at bias + k sBias, its input bound at amax_in + k sAmaxIn and raises amax_out + k sAmaxOut
    // (floats).  Bt = g.B and zero strides: the single-task launch.  Eight launches of 8 samples cost 2-14 % more than one of 64
    // (prologue, tail and launch boundary of a persistent grid: tools/probe/conv_batch_tasks.py)
    int Bt;
    long sW, sBias, sAmaxIn, sAmaxOut;
    // tasks of different frame counts stacked at a common T (mtl_zero_tails): task k's rows t >= widths[k] >> wshift are not computed at
    // all -- the tile index space holds only the ceil(rows / tile rows) leading tile rows of every task (their outputs are left untouched:
    // the caller clears them).  nullptr: every tile of the T x F extent.
    const int* widths;
    int wshift;
#ifdef MTL_X3_PROF
    unsigned long long* prof;   // probe builds only (tools/probe/conv_prof.py): [workgroup][wave][8] accumulated s_memtime intervals
#endif
};
// In-kernel stall breakdown (probe builds: hipcc -DMTL_X3_PROF, never in the product build where the macros are empty): each role
// accumulates s_memtime intervals per phase -- real instruction stream, real operands, the production clock / power state.
#ifdef MTL_X3_PROF
static unsigned long long* g_x3_prof = nullptr;
extern "C" void mtl_x3_prof_set(void* buf) { g_x3_prof = (unsigned long long*)buf; }
#define X3_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define X3_ACC(slot, a, b) prof_acc[slot] += (b) - (a)
#define X3_PROF_DECL unsigned long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define X3_PROF_FLUSH()                                                                                    \
    if (p.prof && (threadIdx.x & 63) == 0) {                                                               \
        for (int k_ = 0; k_ < 8; ++k_) p.prof[((long)blockIdx.x * 16 + (threadIdx.x >> 6)) * 8 + k_] = prof_acc[k_]; \
    }
#else
#define X3_T(v)
#define X3_ACC(slot, a, b)
#define X3_PROF_DECL
#define X3_PROF_FLUSH()
#endif

// ------------------------------------------------------------------ halo-tiled x3 convolution (the one the C ABI dispatches to)
// What the ablation of conv3x3_x3_kernel showed: the consumer side can run 256 TF-equivalent, the producer
// side is bound by (a) re-gathering + re-splitting every input element once per tap and (b) the weight tile per 128 pixels.
// Here a workgroup owns an (8 G) x 16 pixel tile (G pool-aligned 8 x 16 sub-tiles, 4 G consumer waves) and, per 32-channel
// chunk, stages the input HALO once (gather + 3-way split + LDS write) for all nine taps; the consumers address the halo
// with a per-tap offset.  Weight tiles ([piece][K-tile][row][32], double-buffered) are shared by all pixels of the tile.
// Workgroups are PERSISTENT: (tile, chunk) pairs form one sequence of stages, so the producers fetch the next tile's first
// halo under the current tile's last chunk and the consumers' epilogue runs while the producers commit it -- no per-tile
// prologue on the matrix pipe.  G = 2: LDS = halo 324 px x 80 B x 3 planes (76 KiB) + 2 x 3 x BN x 80 B weights (60 KiB at
// BN = 128), 12 waves per CU.
constexpr int XH_HF = 18;                                          // halo width (F) of a 16-wide tile

struct X3Tile {
    int b, n0, t0, f0;
};

inline int device_cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        n = 256;
    return n;
}

template <int G>
__device__ inline int x3_task_rows(const ConvX3P& p, int task) {      // tile rows of a task that has frames of its own
    const int r = ((p.widths[task] >> p.wshift) + 8 * G - 1) / (8 * G);
    return r < p.ntt ? (r < 1 ? 1 : r) : p.ntt;
}

template <int G>
__device__ inline int x3_total_tiles(const ConvX3P& p) {
    if (!p.widths) return p.tiles;
    const int nt = p.g.B / p.Bt;
    int total = 0;
    for (int k = 0; k < nt; ++k) total += p.Bt * p.ntile * x3_task_rows<G>(p, k) * p.ntf;
    return total;
}

// A role's position in the compacted index space (per-task tile rows): a role asks for tiles in rising order, so the walk over the
// tasks -- one load of a frame count each -- advances a few times per kernel, not once per tile.
struct X3Cur {
    int k = 0, lo = 0, hi = -1, ntt = 0;
};

template <int G>
__device__ inline X3Tile x3_tile(const ConvX3P& p, int id, X3Cur& c) {
    X3Tile t;
    int ntt = p.ntt, b0 = 0;
    if (p.widths) {                // compacted index space: task by task, each with its own number of tile rows
        const int per_row = p.Bt * p.ntile * p.ntf, nt = p.g.B / p.Bt;
        if (c.hi < 0 || id < c.lo) {
            c.k = 0;
            c.lo = 0;
            c.ntt = x3_task_rows<G>(p, 0);
            c.hi = per_row * c.ntt;
        }
        while (id >= c.hi && c.k < nt - 1) {
            ++c.k;
            c.lo = c.hi;
            c.ntt = x3_task_rows<G>(p, c.k);
            c.hi = c.lo + per_row * c.ntt;
        }
        id -= c.lo;
        ntt = c.ntt;
        b0 = c.k * p.Bt;
    }
    const int fx = id % p.ntf;
    id /= p.ntf;
    const int ty = id % ntt;
    id /= ntt;
    t.f0 = fx * 16;
    t.t0 = ty * (8 * G);
    t.n0 = id % p.ntile;           // output-channel tile index (x BN at the use site)
    t.b = b0 + id / p.ntile;
    return t;
}

// The wave maximum of mtl_common.h goes through ds_bpermute with six lane-index registers, which the compiler computes once per kernel and
// keeps (or spills) across the matrix loop.  SWZ: the same maximum from ds_swizzle (constant patterns) and two v_readlane, no index register
// -- for the instantiations that have none to spare.  (A maximum does not depend on the order it is taken in: the same bits.)
template <bool SWZ>
__device__ __forceinline__ float x3_wave_max(float v) {
    if constexpr (!SWZ) {
        return wave_max(v);
    } else {
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (1 << 10) | 0x1f)));
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (2 << 10) | 0x1f)));
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (4 << 10) | 0x1f)));
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (8 << 10) | 0x1f)));
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (16 << 10) | 0x1f)));
        return fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)));
    }
}
template <bool SWZ>
__device__ __forceinline__ float x3_amax_read(const float* a) {      // amax_read / amax_raise of mtl_common.h on x3_wave_max
    return x3_wave_max<SWZ>(a[(threadIdx.x & (MTL_AMAX_SLOTS - 1)) * MTL_AMAX_STRIDE]);
}
template <bool SWZ>
__device__ __forceinline__ void x3_amax_raise(float* a, float mx) {
    mx = x3_wave_max<SWZ>(mx);
    float* slot = a + (blockIdx.x & (MTL_AMAX_SLOTS - 1)) * MTL_AMAX_STRIDE;
    if ((threadIdx.x & 63) == 0 && mx > *slot) atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(mx));
}

// The two-piece fp16 instantiations with 64 px x 64 ch consumer waves whose epilogue runs in the SLIM form (kernel header) besides the
// 64-channel data gradients (WN = 1): the forwards of conv2 (BN = 64, WN = 1: ReLU and ReLU + pool) and conv5 (BN = 128, WN = 2: ReLU),
// and conv7's un-pooling data gradient.  A form is listed only while it measures faster than store4x2 / gate4x2 + store4x2g on isolated
// launches (profiles/conv_fwd_epilogue/kernel_ab.txt): conv7's ReLU + pool forward (BN = 128, POOL) compiled to 129 registers without
// scratch in this form too, but ran 1.871 against 1.867 ms, and keeps the epilogue it had.
template <int BN, int G, bool UNPOOL, int EPI, int NP, int WN>
constexpr bool x3h_slim_fwd() {
    return X3H_M16 != 0 && NP == 2 && G == 2 && !UNPOOL &&
           ((BN == 64 && WN == 1 && EPI != EPI_DGRAD) || (BN == 128 && WN == 2 && EPI == EPI_RELU));
}
template <int BN, int G, bool UNPOOL, int EPI, int NP, int WN>
constexpr bool x3h_slim_dg128() {
    return NP == 2 && G == 2 && UNPOOL && EPI == EPI_DGRAD && BN == 128 && WN == 2;
}
// A SLIM epilogue adds ONE 32-bit byte offset per lane to a scalar base: at most 15 frequency positions (a clamped gate row) of `ch`
// channels plus the lane's column inside the wave's 64.  A pure function of the shape; shapes beyond it take the WIDE (64-bit) twin.
constexpr bool x3h_lane_offsets_fit(long ch) { return (15 * ch + 64) * 4 < (1L << 32); }
static_assert(x3h_lane_offsets_fit(128) && x3h_lane_offsets_fit(71582783) && !x3h_lane_offsets_fit(71582784), "just below / at the limit");
static_assert((15 * 71582783L + 63) * 4 + 7 <= 0xffffffffL, "the last byte a lane offset reaches below the limit");

// WN = consumer waves along the output channels of a 128-pixel sub-tile (2 pixel halves x WN): 2 -> each wave owns 64 px x BN/2 ch,
// 1 -> 64 px x BN ch.  The fragment reads of a wave feed TM x TN MFMA groups, (TM + TN) NP ds_read_b128 per TM TN groups: with
// 64 output channels WN = 2 means 3 reads per group (two-piece fp16: LDS 100 % busy at 50 % matrix-pipe load), WN = 1 means 2.
// WIDE: the instantiation's twin with the 64-bit per-element addresses of store4 / store4x2 / gate4 (shapes x3h_lane_offsets_fit refuses)
template <int BN, int G, bool UNPOOL, int EPI, int NP, int WN, bool WIDE = false>
__global__ __launch_bounds__((2 * WN * G + 4) * 64) __attribute__((amdgpu_waves_per_eu(WN == 1 ? 4 : 1)))   // WN = 1: two workgroups per CU
void conv3x3_x3h_kernel(ConvX3P p) {
    // SLIM: 64 x 64 wave tiles whose epilogue has no register to spare.  (a) wave maxima from ds_swizzle (x3_wave_max: no lane-index
    // registers across the matrix loop); (b) the epilogue addresses every access as scalar base + one 32-bit lane offset, with the lane
    // terms re-derived from the lane index inside the epilogue (SLIM_FWD: the ReLU / pool forms, SLIM_DG: the gated form).
    // SLIM_HALO: the halo waves keep their validity bits in one register and re-derive the elements' lane terms at the fetch and at
    // the commit; SLIM_H32: a pooled source is fetched with 32-bit offsets (launcher guard of its own).  Only the dense 64-channel-wave
    // data gradient: the re-derivation sits in the commit, between the two barriers of a halo swap, and cost the forwards 5 %.  The
    // un-pooling forms needed it while they gathered per un-pooled position (14 x (float4 + codes) per thread: conv7's halo waves
    // spilled 56 bytes without it); gathering per pooled element (5 per thread) they compile without scratch and without it.
    constexpr bool SLIM_FWD = !WIDE && x3h_slim_fwd<BN, G, UNPOOL, EPI, NP, WN>();
    constexpr bool SLIM_H32 = WN == 1 && EPI == EPI_DGRAD;
    constexpr bool SLIM_DG = SLIM_H32 || (!WIDE && x3h_slim_dg128<BN, G, UNPOOL, EPI, NP, WN>());
    constexpr bool SLIM_HALO = SLIM_DG && !UNPOOL;
    constexpr bool SLIM = SLIM_DG || SLIM_FWD;
    constexpr int CW = 2 * WN;                                      // consumer waves per 8 x 16 sub-tile
    constexpr int WTM = 64, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
    constexpr int XH_HT = 8 * G + 2, XH_NPIX = XH_HT * XH_HF;      // halo of an (8 G) x 16 tile
    constexpr int XH_APLANE = XH_NPIX * X3_ROWB;                   // one bf16 plane of the halo
    constexpr int NHALO = 3 * 64;                                  // halo threads (producer waves 1-3)
    constexpr int XH_NVA = (XH_NPIX * 8 + NHALO - 1) / NHALO;      // float4 (4 channels) per halo thread and chunk
    constexpr int NCONS = CW * G * 64;                             // consumer threads
    constexpr int BPLANE = BN * 64, BBUF = NP * BPLANE, ABUF = NP * XH_APLANE;   // weights: unpadded swizzled 64-byte rows
    constexpr int NDMA = BBUF / 1024;                              // wave-wide 16-byte DMA instructions per weight tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
    unsigned char* smA = smx;
    unsigned char* smB = smx + ABUF;                               // three stages of BBUF
    const int tid = threadIdx.x;
    const int Cin = p.g.Cin, Cout = p.g.Cout, cch = Cin / BK, nk = 9 * cch;
    const int T = p.g.T, F = p.g.F, Tp = p.g.Tp, Fp = p.g.Fp;
    const int my_tiles = (x3_total_tiles<G>(p) - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    if (my_tiles <= 0) return;                                     // (fewer tiles than workgroups: only with per-task rows)
    const int nstage = my_tiles * cch;                             // stage q = (tile q / cch of this workgroup, chunk q % cch)
    const int nstep = nstage * 9;                                  // step s = stage * 9 + tap; weight stage s % 3

    if (tid >= NCONS + 64) {
        // ------------------------------------------------------------------ halo waves (3): gather, 3-way split, LDS image
        const int ptid = tid - NCONS - 64;
        float sx = NP == 2 ? pow2_scale(x3_amax_read<SLIM>(p.amax_in)) : 1.f;
        int sx_task = 0;
        X3Cur cur_scale, cur_halo;
        auto set_scale = [&](int qc) {          // the operand scale of the task that stage qc's tile belongs to
            if (NP != 2 || p.Bt >= p.g.B) return;
            const int tk = x3_tile<G>(p, blockIdx.x + (qc / cch) * gridDim.x, cur_scale).b / p.Bt;
            if (tk != sx_task) {
                sx_task = tk;
                sx = pow2_scale(x3_amax_read<SLIM>(p.amax_in + tk * p.sAmaxIn));
            }
        };
        // UNPOOL: an element is a POOLED source element -- pooling window (wr, wc) of the (4 G + 2) x 10 that the halo touches (tile origins
        // are even: halo row ht lies in window (ht + 1) >> 1 at row parity (ht + 1) & 1, columns alike), channels c4 .. c4 + 3 -- fetched
        // and split once and committed to the up to four halo pixels of its window (edge windows have one row / column inside the halo).
        constexpr int XW_WF = XH_HF / 2 + 1, XW_NW = (XH_HT / 2 + 1) * XW_WF;     // windows along F; windows per halo
        constexpr int XW_NVA = (XW_NW * 8 + NHALO - 1) / NHALO;                  // G = 2: 800 elements, at most 5 per thread (un-pooled: 2592, 14)
        constexpr int NVA = UNPOOL ? XW_NVA : XH_NVA;
        float4 hv[NVA];
        uchar4 ha[NVA];
        unsigned hm[SLIM_HALO || UNPOOL ? 1 : XH_NVA];   // SLIM_HALO / UNPOOL: the validity bits of all elements in hm[0]
        auto fetch_halo = [&](int q) {          // stage q: channels c*32 .. +31 of the halo pixels of its tile
            const int j = q / cch, c = q - j * cch;
            const X3Tile tl = x3_tile<G>(p, blockIdx.x + j * gridDim.x, cur_halo);
            int pt = ptid;                      // (SLIM_HALO: the elements' lane terms are derived here, not kept -- spilled -- from the prologue)
            if constexpr (SLIM_HALO) asm volatile("" : "+v"(pt));
            if constexpr (UNPOOL) {
                // A window inside Tp x Fp has all four of its positions inside T x F (Tp = T / 2, Fp = F / 2: the C ABI derives them),
                // and a position outside every such window -- beyond the image, or the last row / column of an odd extent -- is zero.
                const int tw0 = (tl.t0 >> 1) - 1, fw0 = (tl.f0 >> 1) - 1;
#pragma unroll
                for (int i = 0; i < XW_NVA; ++i) {
                    const int e = pt + i * NHALO;
                    const int w = min(e >> 3, XW_NW - 1), c4 = (e & 7) * 4;
                    const int wr = w / XW_WF, wc = w - wr * XW_WF;
                    const int tp = tw0 + wr, fp = fw0 + wc;
                    const bool ok = (e >> 3) < XW_NW && (unsigned)tp < (unsigned)Tp && (unsigned)fp < (unsigned)Fp;
                    const int tpc = max(min(tp, Tp - 1), 0), fpc = max(min(fp, Fp - 1), 0);
                    if constexpr (SLIM_H32) {   // scalar base of the (sample, chunk) + one 32-bit offset for both loads: no 64-bit address pair per element
                        const long sbase = (long)__builtin_amdgcn_readfirstlane(tl.b) * Tp * Fp * Cin + c * BK;
                        const unsigned o = (unsigned)((tpc * Fp + fpc) * Cin + c4);
                        ha[i] = *reinterpret_cast<const uchar4*>(p.am_in + sbase + o);
                        hv[i] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.x + sbase) + o * 4u);
                    } else {
                        const long o = (((long)tl.b * Tp + tpc) * Fp + fpc) * Cin + c * BK + c4;
                        ha[i] = *reinterpret_cast<const uchar4*>(p.am_in + o);
                        hv[i] = *reinterpret_cast<const float4*>(p.x + o);
                    }
                    hm[0] = i ? hm[0] | ((ok ? 1u : 0u) << i) : (ok ? 1u : 0u);
                }
                return;
            }
#pragma unroll
            for (int i = 0; i < XH_NVA; ++i) {
                const int e = pt + i * NHALO;
                const int hp = min(e >> 3, XH_NPIX - 1), c4 = (e & 7) * 4;
                const int ht = hp / XH_HF, hf = hp - ht * XH_HF;
                const int ts = tl.t0 + ht - 1, fs = tl.f0 + hf - 1;
                const bool ok = (e >> 3) < XH_NPIX && (unsigned)ts < (unsigned)T && (unsigned)fs < (unsigned)F;
                const int tc = min(max(ts, 0), T - 1), fc = min(max(fs, 0), F - 1);
                hv[i] = *reinterpret_cast<const float4*>(p.x + (((long)tl.b * T + tc) * F + fc) * Cin + c * BK + c4);
                if constexpr (SLIM_HALO) hm[0] = i ? hm[0] | ((ok ? 1u : 0u) << i) : (ok ? 1u : 0u);
                else hm[i] = ok ? 1u : 0u;
            }
        };
        // (Splitting ahead of the swap barrier so that only the ds_writes sit between the two barriers was tried: the 84
        // extra live registers spill under the 168-VGPR cap of a 12-wave workgroup and every launch gets 15-40 % slower.)
        auto commit_halo = [&]() {
            int pt = ptid;
            if constexpr (SLIM_HALO) asm volatile("" : "+v"(pt));
            if constexpr (UNPOOL) {
#pragma unroll
                for (int i = 0; i < XW_NVA; ++i) {
                    const int e = pt + i * NHALO;
                    if ((e >> 3) >= XW_NW) continue;
                    const int wr = (e >> 3) / XW_WF, wc = (e >> 3) - wr * XW_WF;
                    uint2 pc[NP];
                    split_x4<NP>(hv[i], sx, pc);                                  // once per pooled value: a position takes the piece words or zero
                    const uchar4 a = (hm[0] >> i) & 1u ? ha[i] : make_uchar4(255, 255, 255, 255);      // (no window there: no position matches)
                    unsigned char* dst = smA + ((2 * wr - 1) * XH_HF + 2 * wc - 1) * X3_ROWB + (e & 7) * 8;    // halo pixel of position 0
#pragma unroll
                    for (int pos = 0; pos < 4; ++pos) {                           // pos = ((f & 1) << 1) | (t & 1): what the arg-max code names
                        const int dr = pos & 1, dc = pos >> 1;
                        if ((dr ? wr < XH_HT / 2 : wr > 0) && (dc ? wc < XW_WF - 1 : wc > 0)) {        // the position lies inside the halo
                            const unsigned m0 = (a.x == pos ? 0xffffu : 0u) | (a.y == pos ? 0xffff0000u : 0u);
                            const unsigned m1 = (a.z == pos ? 0xffffu : 0u) | (a.w == pos ? 0xffff0000u : 0u);
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                *reinterpret_cast<uint2*>(dst + (dr * XH_HF + dc) * X3_ROWB + q * XH_APLANE) = make_uint2(pc[q].x & m0, pc[q].y & m1);
                        }
                    }
                }
                return;
            }
#pragma unroll
            for (int i = 0; i < XH_NVA; ++i) {
                const int e = pt + i * NHALO;
                if ((e >> 3) >= XH_NPIX) continue;
                const bool ok = SLIM_HALO ? (hm[0] >> i) & 1u : hm[i] & 1u;
                const float4 v = mask4(hv[i], ok ? 15u : 0u);
                uint2 pc[NP];
                split_x4<NP>(v, sx, pc);
                unsigned char* dst = smA + (e >> 3) * X3_ROWB + (e & 7) * 8;
#pragma unroll
                for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(dst + q * XH_APLANE) = pc[q];
            }
        };
        const bool doA = !(p.dbg & 2);
        X3_PROF_DECL;
        X3_T(h0);
        if (doA) fetch_halo(0);
        set_scale(0);
        if (doA) commit_halo();
        if (nstage > 1 && doA) fetch_halo(1);
        __syncthreads();                                       // halo of stage 0 (and the weights of step 0) are visible
        X3_T(h1);
        X3_ACC(0, h0, h1);                                     // prologue
#pragma unroll 1
        for (int q = 0; q < nstage; ++q) {
            X3_T(a0);
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) __syncthreads();
            X3_T(a1);
            X3_ACC(1, a0, a1);                                 // nine tap barriers
            if (q + 1 < nstage) {
                set_scale(q + 1);
                if (doA) commit_halo();                        // nobody reads the halo between these two barriers
                X3_T(a2);
                X3_ACC(2, a1, a2);                             // commit (includes the wait for the fetch)
                if (q + 2 < nstage && doA) fetch_halo(q + 2);  // a whole stage of flight time
                X3_T(a3);
                X3_ACC(3, a2, a3);                             // fetch issue
                __syncthreads();
                X3_T(a4);
                X3_ACC(4, a3, a4);                             // closing barrier of the swap
            }
        }
        X3_PROF_FLUSH();
        return;
    }
    if (tid >= NCONS) {
        // ------------------------------------------------------------------ weight wave: global_load_lds only
        // The K-tile of step s (tap * cch + chunk, output-channel tile n0) is one contiguous, pre-swizzled 3 x BN x 64 B
        // block per piece; NDMA wave-wide 16-byte DMA instructions move it into stage s % 3 with no registers and no
        // ds_write.  This wave's vmcnt counts only those DMAs (in order), so "tile s + 1 has landed" is vmcnt(NDMA) right
        // after the tile of step s + 2 was issued: two steps of flight time, never a drain.  Raw s_barrier: __syncthreads
        // would add vmcnt(0).
        const int lane = tid & 63;
        const bool doB = !(p.dbg & 4);
        int dma_j = -1, dma_n0 = 0;
        X3Cur cur_dma;
        const unsigned char* dma_w3 = p.w3;
        auto dma = [&](int s_) {
            const int q = s_ / 9, tap = s_ - q * 9;
            const int j = q / cch, c = q - j * cch;
            if (j != dma_j && (p.ntile != 1 || p.Bt < p.g.B)) {      // (once per tile: the tile's channel block and its task's weights)
                const X3Tile tl = x3_tile<G>(p, blockIdx.x + j * gridDim.x, cur_dma);
                dma_n0 = tl.n0 * BN;
                dma_w3 = p.w3 + (tl.b / p.Bt) * p.sW;
                dma_j = j;
            }
            const int n0 = dma_n0;
            const unsigned char* w3 = dma_w3;
            const int kt = tap * cch + c;
            unsigned char* dst = smB + (s_ % 3) * BBUF;            // scalar ALU
#pragma unroll
            for (int i = 0; i < NDMA; ++i) {
                const int piece = i / (BN / 16), r16 = i - piece * (BN / 16);       // 16 rows (1 KiB) per instruction
                const unsigned char* g = w3 + (((long)piece * nk + kt) * Cout + n0 + r16 * 16) * 64 + lane * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                 (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
            }
        };
        if (doB) {
            dma(0);
            if (nstep > 1) dma(1);
        }
        if (nstep > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        int tap = 0, q = 0;
        X3_PROF_DECL;
#pragma unroll 1
        for (int s_ = 0; s_ < nstep; ++s_) {
            // stage (s_ + 2) % 3 was read at step s_ - 1, and every consumer has passed that step's barrier
            X3_T(w0);
            if (s_ + 2 < nstep) {
                if (doB) dma(s_ + 2);
                X3_T(w1);
                X3_ACC(0, w0, w1);                                                // issue
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");      // tile s_ + 1 is in LDS
                X3_T(w2);
                X3_ACC(1, w1, w2);                                                // landing wait
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            X3_T(w3);
            __builtin_amdgcn_s_barrier();
            X3_T(w4);
            X3_ACC(2, w3, w4);                                                    // step barrier
            if (++tap == 9) {
                tap = 0;
                if (++q < nstage) __builtin_amdgcn_s_barrier();                   // the halo swap
                X3_T(w5);
                X3_ACC(3, w4, w5);
            }
        }
        X3_PROF_FLUSH();
        return;
    }

    // ---------------------------------------------------------------------- consumers (G sub-tiles x (2 x 2) waves)
    const int lane = tid & 63, wave = tid >> 6;
    const int grp = wave / CW, w4 = wave % CW;
    const int wm = w4 / WN, wn = w4 % WN, l31 = lane & 31, hi = lane >> 5;
    // M16 (round 4): the wave's 64 x WTN tile as 4 x (WTN / 16) tiles of v_mfma_f32_16x16x32: the same 64 accumulator registers, one 16-byte
    // fragment per lane covers all 32 k of a chunk (lane = row (lane & 15), k-quarter (lane >> 4)).  Under the package power limit the chip
    // sustains 9-12 % more LDS-fed matrix work in this shape than in 32 x 32 x 16 (tools/probe/mfma_shape.py): half the accumulator traffic
    // per flop.  A tile's 4 registers are 4 consecutive tile rows = one pooling window, like a register group of the 32 x 32 layout.
    // (conv5's data gradient -- 64 output channels, 16 x 16 pixel tiles, no un-pooling -- measured 4 % slower in this form with 32-channel waves
    // and keeps 32 x 32 x 16; with 64-channel waves this form is the faster one, X3H_DG5)
    constexpr bool M16 = X3H_M16 != 0 && !(BN == 64 && G == 2 && (WN == 2 || X3H_DG5 != 2) && EPI == EPI_DGRAD && !UNPOOL);
    constexpr int TM16 = WTM / 16, TN16 = WTN / 16;
    // WN = 1 data-gradient epilogue: accumulator groups per batch of gate loads.  16 x 16 x 32: one 16-pixel row block (2 groups x 8 registers, two
    // batches live; 4 groups spill 80-96 bytes); 32 x 32 x 16: one group of 4 registers (2 groups: 16 bytes of scratch, 4: 80)
    constexpr int DGB16 = 2, DGB32 = 1;
    f32x16 acc[M16 ? 1 : TM][M16 ? 1 : TN];
    f32x4 acc4[M16 ? TM16 : 1][M16 ? TN16 : 1];
    const int l15 = lane & 15, q4 = lane >> 4;
    float inv = 1.f, mx = 0.f;                                 // NP = 2: 1 / (activation scale x weight scale); running bound of max|y|
    if (NP == 2) inv = 1.f / (pow2_scale(x3_amax_read<SLIM>(p.amax_in)) * *reinterpret_cast<const float*>(p.w3 + (long)NP * nk * Cout * 64));
    int cur_task = 0;                                          // (several tasks per launch: the task of the tile being finished)
    X3Cur cur_epi;
    const float* bias_t = p.bias;
    // |relu(v + b)| <= |v| + |b| (pooling takes a maximum of those); dgrad: |gate v| <= |v|: the bound of a task's output leaves when
    // the workgroup's tiles move on to the next task (its tile sequence visits the tasks in order) and at the end
    auto raise_bound = [&]() {
        if (!p.amax_out) return;
        float bmax = 0.f;
        if constexpr (SLIM_FWD) {          // the task's bias from its index and the lane's column from a re-read lane index: kept from the
            int c15;                       // prologue, the per-task pointer and the lane's bias addresses are spilled across the matrix loop
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(c15));
            const float* bias_k = p.bias + (long)cur_task * p.sBias + wn * WTN + 2 * (c15 & 15);
#pragma unroll
            for (int jn = 0; jn < TN16; ++jn)
                for (int nt = 0; nt < p.ntile; ++nt) bmax = fmaxf(bmax, fabsf(bias_k[nt * BN + (jn >> 1) * 32 + (jn & 1)]));
        } else
        if (EPI != EPI_DGRAD) {
            if (M16) {
#pragma unroll
                for (int jn = 0; jn < TN16; ++jn)
                    for (int nt = 0; nt < p.ntile; ++nt)
                        bmax = fmaxf(bmax, fabsf(bias_t[nt * BN + wn * WTN + (jn >> 1) * 32 + 2 * l15 + (jn & 1)]));
            } else
#pragma unroll
            for (int jn = 0; jn < TN; ++jn)
                for (int nt = 0; nt < p.ntile; ++nt) bmax = fmaxf(bmax, fabsf(bias_t[nt * BN + wn * WTN + jn * 32 + l31]));
        }
        x3_amax_raise<SLIM>(p.amax_out + cur_task * p.sAmaxOut, mx + bmax);
    };
    int abase[TM];                                             // byte offset of this lane's pixel (tap centre) in the halo plane
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int t, f;
        tile_row_to_tf(wm * WTM + i * 32 + l31, t, f);
        abase[i] = ((t + grp * 8 + 1) * XH_HF + (f + 1)) * X3_ROWB + hi * 16;
#ifdef X3_FAKE_A
        abase[i] = (XH_HF + 1 + l31 + i * 32 + grp * 64) * X3_ROWB + hi * 16;     // probe build: conflict-free (wrong) fragment addresses
#endif
    }
    int abase16[M16 ? TM16 : 1];
    if (M16) {
#pragma unroll
        for (int i = 0; i < TM16; ++i) {
            int t, f;
            tile_row_to_tf(wm * WTM + i * 16 + l15, t, f);
            abase16[i] = ((t + grp * 8 + 1) * XH_HF + (f + 1)) * X3_ROWB + q4 * 16;
        }
    }
    // tile 2k of a 32-channel block holds its EVEN channels, tile 2k + 1 the odd ones (weight row 32 k + 2 l15 + parity): a lane owns an
    // adjacent channel pair of each block, so the epilogues move 8 bytes per lane and pixel = 128 contiguous bytes per 16 lanes
    const unsigned char* bBase16 = smB + (wn * WTN + 2 * l15) * 64 + ((q4 ^ ((l15 >> 1) & 3)) * 16);
    const unsigned char* bBase = smB + (wn * WTN + l31) * 64;
    int bsw[BK / 16];                                          // swizzled position of this lane's 16-byte chunk per k-step
#pragma unroll
    for (int st = 0; st < BK / 16; ++st) bsw[st] = (((st * 2 + hi) ^ ((l31 >> 2) & 3))) * 16;
    __syncthreads();
    int bst = 0;                                               // weight stage of the current step (step % 3)
    X3_PROF_DECL;
    X3_T(k0);
#pragma unroll 1
    for (int j = 0; j < my_tiles; ++j) {
        if (M16) {
#pragma unroll
            for (int i = 0; i < TM16; ++i)
#pragma unroll
                for (int jn = 0; jn < TN16; ++jn) acc4[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[i][jn][v] = 0.f;
        }
#pragma unroll 1
        for (int c = 0; c < cch; ++c) {
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap, bst = bst == 2 ? 0 : bst + 1) {
                const int kh = tap / 3, kw = tap - kh * 3;
                const int toff = ((kw - 1) * XH_HF + (kh - 1)) * X3_ROWB;
                const unsigned char* bS = bBase + bst * BBUF;
                X3_T(c0);
                if (M16) {
                    const unsigned char* bS16 = bBase16 + bst * BBUF;
                    uint4 b16[TN16][NP];
#pragma unroll
                    for (int jn = 0; jn < TN16; ++jn)
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc)
                            b16[jn][pc] = *reinterpret_cast<const uint4*>(bS16 + pc * BPLANE + ((jn >> 1) * 32 + (jn & 1)) * 64);
                    constexpr int IH = X3H_IH ? X3H_IH : 2;         // row blocks per fragment batch: IH NP fragments live beside the weights'
#pragma unroll
                    for (int ih = 0; ih < TM16; ih += IH) {
                        uint4 a16[IH][NP];
#pragma unroll
                        for (int i = 0; i < IH; ++i)
#pragma unroll
                            for (int pc = 0; pc < NP; ++pc)
                                a16[i][pc] = *reinterpret_cast<const uint4*>(smA + pc * XH_APLANE + abase16[ih + i] + toff);
#pragma unroll
                        for (int i = 0; i < IH; ++i)
#pragma unroll
                            for (int jn = 0; jn < TN16; ++jn) acc4[ih + i][jn] = Split<NP>::mfma16(a16[i], b16[jn], acc4[ih + i][jn]);
                    }
                } else
#pragma unroll
                for (int st = 0; st < BK / 16; ++st) {
                    uint4 a[TM][NP], bb[TN][NP];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc)
                            a[i][pc] = *reinterpret_cast<const uint4*>(smA + pc * XH_APLANE + abase[i] + toff + st * 32);
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc)
                            bb[jn][pc] = *reinterpret_cast<const uint4*>(bS + pc * BPLANE + jn * 32 * 64 + bsw[st]);
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int jn = 0; jn < TN; ++jn) acc[i][jn] = Split<NP>::mfma(a[i], bb[jn], acc[i][jn]);
                }
                X3_T(c1);
                X3_ACC(0, c0, c1);                             // reads + matrix instructions issued
                __syncthreads();
                X3_T(c2);
                X3_ACC(1, c1, c2);                             // step barrier (drain + wait for the slowest wave)
            }
            X3_T(e0);
            if (c + 1 == cch && !(p.dbg & 8)) {
                // epilogue (no LDS): same row -> (pool window, position) walk as Engine::finish with this wave's sub-tile
                // origin; it runs while the producers commit the next tile's halo
                // (the tile index goes through an opaque asm so that the per-lane output addresses are computed HERE: hoisted
                // above the MFMA loops they were spilled per tile, and the scratch traffic doubled the dgrad kernels' HBM writes)
                int jj = j;
                asm volatile("" : "+s"(jj));
                const X3Tile tl = x3_tile<G>(p, blockIdx.x + jj * gridDim.x, cur_epi);
                const int ts0 = tl.t0 + grp * 8, n0 = tl.n0 * BN;
                if (p.Bt < p.g.B) {
                    const int tk = tl.b / p.Bt;
                    if (tk != cur_task) {
                        raise_bound();
                        mx = 0.f;
                        cur_task = tk;
                        bias_t = p.bias + tk * p.sBias;
                        if (NP == 2)
                            inv = 1.f / (pow2_scale(x3_amax_read<SLIM>(p.amax_in + tk * p.sAmaxIn)) *
                                         *reinterpret_cast<const float*>(p.w3 + tk * p.sW + (long)NP * nk * Cout * 64));
                    }
                }
                auto walk = [&](auto&& epi) {
                    if (M16) {
#pragma unroll
                        for (int i = 0; i < TM16; ++i)
#pragma unroll
                            for (int jn = 0; jn < TN16; jn += 2) {
                                float v0[4], v1[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    v0[k] = NP == 2 ? acc4[i][jn][k] * inv : acc4[i][jn][k];
                                    v1[k] = NP == 2 ? acc4[i][jn + 1][k] * inv : acc4[i][jn + 1][k];
                                    mx = fmaxf(mx, fmaxf(fabsf(v0[k]), fabsf(v1[k])));
                                }
                                epi.store4x2(wm * WTM + i * 16 + 4 * q4, wn * WTN + (jn >> 1) * 32 + 2 * l15, v0, v1);
                            }
                        return;
                    }
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                float v[4] = {acc[i][jn][4 * g], acc[i][jn][4 * g + 1], acc[i][jn][4 * g + 2], acc[i][jn][4 * g + 3]};
                                if (NP == 2) {
#pragma unroll
                                    for (int k = 0; k < 4; ++k) v[k] *= inv;
                                }
                                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                                epi.store4(wm * WTM + i * 32 + 8 * g + 4 * hi, wn * WTN + jn * 32 + l31, v);
                            }
                };
                if constexpr (SLIM_FWD) {
                    // EpiConvRelu::store4x2 / EpiConvPool::store4x2 in the SLIM addressing form (the data-gradient branch below explains it):
                    // the sample, the tile, the wave's rows and channel block, the accumulator group and the task are wave-uniform, so a store
                    // is a scalar base + ONE 32-bit lane offset (the pooled value and its arg-max pair share it: x 4 and x 1), the bias pairs
                    // of the wave's two 32-channel blocks come from a scalar base + the lane's column and are requested once per tile, ahead
                    // of the first group.  Per element the arithmetic and its order are store4x2's: * inv, max|v|, + bias, max(., 0), the
                    // first maximum in window order, the same predicates.
                    int el;
                    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(el));
                    const int sb = __builtin_amdgcn_readfirstlane(tl.b), sf0 = __builtin_amdgcn_readfirstlane(tl.f0);
                    const int st0 = __builtin_amdgcn_readfirstlane(ts0 + 4 * wm), sn0 = __builtin_amdgcn_readfirstlane(n0 + wn * WTN);
                    const float* sbias = p.bias + ((long)__builtin_amdgcn_readfirstlane(cur_task) * p.sBias + sn0);
                    const unsigned lcol = 2 * (el & 15);
                    f32x2v bb[TN16 / 2];
#pragma unroll
                    for (int jp = 0; jp < TN16 / 2; ++jp)
                        bb[jp] = *reinterpret_cast<const f32x2v*>(reinterpret_cast<const char*>(sbias + jp * 32) + lcol * 4u);
                    if constexpr (EPI == EPI_RELU) {
                        // rows of group i: t = st0 + 2 (i >> 1) + (k & 1); f = sf0 + fu + fl (fu: group and k, fl: lane)
                        const int fl = 2 * (el >> 4);
                        const unsigned so = (unsigned)(fl * Cout + lcol) * 4u;
#pragma unroll
                        for (int i = 0; i < TM16; ++i)
#pragma unroll
                            for (int jp = 0; jp < TN16 / 2; ++jp)
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const float v0 = acc4[i][2 * jp][k] * inv, v1 = acc4[i][2 * jp + 1][k] * inv;
                                    mx = fmaxf(mx, fmaxf(fabsf(v0), fabsf(v1)));
                                    asm volatile("" : "+v"(mx));      // (pinned, as in the data-gradient branch)
                                    const int t = st0 + 2 * (i >> 1) + (k & 1), fu = 8 * (i & 1) + (k >> 1);
                                    const f32x2v o = {fmaxf(v0 + bb[jp].x, 0.f), fmaxf(v1 + bb[jp].y, 0.f)};
                                    if (t < T && sf0 + fu + fl < F)
                                        __builtin_nontemporal_store(o, reinterpret_cast<f32x2v*>(reinterpret_cast<char*>(
                                            p.y + ((((long)sb * T + t) * F + sf0 + fu) * Cout + sn0 + jp * 32)) + so));
                                }
                    } else {
                        // window of group i: tp = st0 / 2 + (i >> 1); fp = sf0 / 2 + 4 (i & 1) + (lane >> 4)
                        const int flp = el >> 4;
                        const unsigned so = (unsigned)(flp * Cout) + lcol;          // in elements
#pragma unroll
                        for (int i = 0; i < TM16; ++i)
#pragma unroll
                            for (int jp = 0; jp < TN16 / 2; ++jp) {
                                float v0[4], v1[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    v0[k] = acc4[i][2 * jp][k] * inv;
                                    v1[k] = acc4[i][2 * jp + 1][k] * inv;
                                    mx = fmaxf(mx, fmaxf(fabsf(v0[k]), fabsf(v1[k])));
                                }
                                asm volatile("" : "+v"(mx));
                                const int tp = (st0 >> 1) + (i >> 1), fpu = (sf0 >> 1) + 4 * (i & 1);
                                if (tp < Tp && fpu + flp < Fp) {
                                    float best0 = fmaxf(v0[0] + bb[jp].x, 0.f), best1 = fmaxf(v1[0] + bb[jp].y, 0.f);
                                    int idx0 = 0, idx1 = 0;
#pragma unroll
                                    for (int k = 1; k < 4; ++k) {
                                        const float x0 = fmaxf(v0[k] + bb[jp].x, 0.f), x1 = fmaxf(v1[k] + bb[jp].y, 0.f);
                                        if (x0 > best0) best0 = x0, idx0 = k;
                                        if (x1 > best1) best1 = x1, idx1 = k;
                                    }
                                    const long e = (((long)sb * Tp + tp) * Fp + fpu) * Cout + sn0 + jp * 32;
                                    *reinterpret_cast<float2*>(reinterpret_cast<char*>(p.y + e) + so * 4u) = make_float2(best0, best1);
                                    *reinterpret_cast<unsigned short*>(p.am_out + e + so) = (unsigned short)(idx0 | (idx1 << 8));
                                }
                            }
                    }
                } else if (EPI == EPI_RELU) {
                    walk(EpiConvRelu{p.y, bias_t, tl.b, ts0, tl.f0, T, F, Cout, n0});
                } else if (EPI == EPI_POOL) {
                    walk(EpiConvPool{p.y, p.am_out, bias_t, tl.b, ts0, tl.f0, Tp, Fp, Cout, n0});
                } else if constexpr (SLIM_DG) {
                    // 64 px x 64 ch wave tiles under 128 registers: 64 accumulators leave no room for all 64 gate values and a 64-bit address
                    // per load and store.  (a) Addresses: everything but the lane's own column / frequency term is wave-uniform (the tile,
                    // the wave's rows, the accumulator group), so every access is a scalar base + ONE 32-bit lane offset, and the lane terms
                    // come from an opaque copy of the lane index -- kept from the prologue they would be spilled across the matrix loop, like
                    // the tile's (above).  (b) Gate values: in batches of GB accumulator groups, batch k + 1 requested before batch k is
                    // stored (act and dx may alias as far as the compiler knows, so no load moves above the stores of batch k - 1): one
                    // batch of loads in flight under the other's stores, 2 x 16 gate registers.  Per element the arithmetic and the
                    // addresses are those of EpiConvDgrad::gate4* / store4*g.
                    int el;
                    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(el));
                    const int sb = __builtin_amdgcn_readfirstlane(tl.b), sf0 = __builtin_amdgcn_readfirstlane(tl.f0);
                    const int st0 = __builtin_amdgcn_readfirstlane(ts0 + 4 * wm), sn0 = __builtin_amdgcn_readfirstlane(n0 + wn * WTN);
                    // rows of the wave's group at 32-row block ib: t = st0 + 2 ib + (j & 1); f = sf0 + fu + fl (fu: group and j, fl: lane)
                    auto gate_base = [&](int t, int cb) {          // clamped row, columns from cb
                        return reinterpret_cast<const char*>(p.act + ((((long)sb * T + min(t, T - 1)) * F + sf0) * Cout + sn0 + cb));
                    };
                    auto out_base = [&](int t, int fu, int cb) {
                        return reinterpret_cast<char*>(p.y + ((((long)sb * T + t) * F + sf0 + fu) * Cout + sn0 + cb));
                    };
                    if constexpr (M16) {
                        constexpr int NG = TM16 * (TN16 / 2);                     // groups: 4 rows x one channel pair of a 32-channel block
                        constexpr int GB = DGB16, NB = NG / GB;                   // groups per batch
                        static_assert(NG % GB == 0, "whole batches");
                        const int fl = 2 * (el >> 4);
                        const unsigned lcol = 2 * (el & 15);
                        const unsigned so = (unsigned)(fl * Cout + lcol) * 4u;
                        f32x2v gate16[NB > 1 ? 2 : 1][GB][4];
                        auto load_gates = [&](int bt) {
#pragma unroll
                            for (int e = 0; e < GB; ++e) {
                                const int u = bt * GB + e, i = u / (TN16 / 2), jp = u % (TN16 / 2);
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const int fc = min(sf0 + 8 * (i & 1) + (k >> 1) + fl, F - 1) - sf0;
                                    gate16[bt & 1][e][k] = __builtin_nontemporal_load(reinterpret_cast<const f32x2v*>(
                                        gate_base(st0 + 2 * (i >> 1) + (k & 1), jp * 32) + (unsigned)(fc * Cout + lcol) * 4u));
                                }
                            }
                        };
                        load_gates(0);
#pragma unroll
                        for (int bt = 0; bt < NB; ++bt) {
                            if (bt + 1 < NB) load_gates(bt + 1);
#pragma unroll
                            for (int e = 0; e < GB; ++e) {
                                const int u = bt * GB + e, i = u / (TN16 / 2), jp = u % (TN16 / 2);
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const float v0 = NP == 2 ? acc4[i][2 * jp][k] * inv : acc4[i][2 * jp][k];
                                    const float v1 = NP == 2 ? acc4[i][2 * jp + 1][k] * inv : acc4[i][2 * jp + 1][k];
                                    mx = fmaxf(mx, fmaxf(fabsf(v0), fabsf(v1)));
                                    asm volatile("" : "+v"(mx));      // (pinned: sunk to the end of the epilogue the maxima keep every scaled value live)
                                    const int t = st0 + 2 * (i >> 1) + (k & 1), fu = 8 * (i & 1) + (k >> 1);
                                    const f32x2v m = gate16[bt & 1][e][k];
                                    const f32x2v o = {m.x > 0.f ? v0 : 0.f, m.y > 0.f ? v1 : 0.f};
                                    if (t < T && sf0 + fu + fl < F)
                                        __builtin_nontemporal_store(o, reinterpret_cast<f32x2v*>(out_base(t, fu, jp * 32) + so));
                                }
                            }
                        }
                    } else {
                        constexpr int NG = TM * TN * 4;                           // groups: 4 rows x one channel of a 32 x 32 tile
                        constexpr int GB = DGB32, NB = NG / GB;
                        static_assert(NG % GB == 0, "whole batches");
                        const int fl = 2 * (el >> 5);
                        const unsigned lcol = el & 31;
                        const unsigned so = (unsigned)(fl * Cout + lcol) * 4u;
                        float gate[NB > 1 ? 2 : 1][GB][4];
                        auto load_gates = [&](int bt) {
#pragma unroll
                            for (int e = 0; e < GB; ++e) {
                                const int u = bt * GB + e, i = u / (TN * 4), jn = (u >> 2) % TN, g = u & 3;
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const int fc = min(sf0 + 4 * g + (k >> 1) + fl, F - 1) - sf0;
                                    gate[bt & 1][e][k] = __builtin_nontemporal_load(reinterpret_cast<const float*>(
                                        gate_base(st0 + 2 * i + (k & 1), jn * 32) + (unsigned)(fc * Cout + lcol) * 4u));
                                }
                            }
                        };
                        load_gates(0);
#pragma unroll
                        for (int bt = 0; bt < NB; ++bt) {
                            if (bt + 1 < NB) load_gates(bt + 1);
#pragma unroll
                            for (int e = 0; e < GB; ++e) {
                                const int u = bt * GB + e, i = u / (TN * 4), jn = (u >> 2) % TN, g = u & 3;
                                float v[4] = {acc[i][jn][4 * g], acc[i][jn][4 * g + 1], acc[i][jn][4 * g + 2], acc[i][jn][4 * g + 3]};
                                if (NP == 2) {
#pragma unroll
                                    for (int k = 0; k < 4; ++k) v[k] *= inv;
                                }
                                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                                asm volatile("" : "+v"(mx));
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const int t = st0 + 2 * i + (k & 1), fu = 4 * g + (k >> 1);
                                    if (t < T && sf0 + fu + fl < F)
                                        __builtin_nontemporal_store(gate[bt & 1][e][k] > 0.f ? v[k] : 0.f,
                                                                    reinterpret_cast<float*>(out_base(t, fu, jn * 32) + so));
                                }
                            }
                        }
                    }
                } else {
                    const EpiConvDgrad epi{p.y, p.act, tl.b, ts0, tl.f0, T, F, Cout, n0};
                    if (M16) {
                        f32x2v gate16[TM16][TN16 / 2][4];      // all gate values of the wave in flight together
#pragma unroll
                        for (int i = 0; i < TM16; ++i)
#pragma unroll
                            for (int jp = 0; jp < TN16 / 2; ++jp) epi.gate4x2(wm * WTM + i * 16 + 4 * q4, wn * WTN + jp * 32 + 2 * l15, gate16[i][jp]);
#pragma unroll
                        for (int i = 0; i < TM16; ++i)
#pragma unroll
                            for (int jp = 0; jp < TN16 / 2; ++jp) {
                                float v0[4], v1[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    v0[k] = NP == 2 ? acc4[i][2 * jp][k] * inv : acc4[i][2 * jp][k];
                                    v1[k] = NP == 2 ? acc4[i][2 * jp + 1][k] * inv : acc4[i][2 * jp + 1][k];
                                    mx = fmaxf(mx, fmaxf(fabsf(v0[k]), fabsf(v1[k])));
                                }
                                epi.store4x2g(wm * WTM + i * 16 + 4 * q4, wn * WTN + jp * 32 + 2 * l15, v0, v1, gate16[i][jp]);
                            }
                    } else {
                    float gate[TM][TN][4][4];                  // all gate values of the wave in flight together
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                epi.gate4(wm * WTM + i * 32 + 8 * g + 4 * hi, wn * WTN + jn * 32 + l31, gate[i][jn][g]);
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                float v[4] = {acc[i][jn][4 * g], acc[i][jn][4 * g + 1], acc[i][jn][4 * g + 2], acc[i][jn][4 * g + 3]};
                                if (NP == 2) {
#pragma unroll
                                    for (int k = 0; k < 4; ++k) v[k] *= inv;
                                }
                                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                                epi.store4g(wm * WTM + i * 32 + 8 * g + 4 * hi, wn * WTN + jn * 32 + l31, v, gate[i][jn][g]);
                            }
                    }
                }
            }
            X3_T(e1);
            X3_ACC(2, e0, e1);                                 // epilogue (issue)
            if (j * cch + c + 1 < nstage) __syncthreads();     // the producers replaced the halo between these two barriers
            X3_T(e2);
            X3_ACC(3, e1, e2);                                 // swap barrier
        }
    }
    X3_T(k1);
    X3_ACC(4, k0, k1);                                         // whole main loop
    X3_PROF_FLUSH();
    raise_bound();
}

template <int BN, int G, bool UNPOOL, int EPI, int NP, int WN = 2, bool WIDE = false>
int launch_conv_x3h(ConvX3P p, int Te, int Fe, hipStream_t s) {
    // the SLIM epilogues of the forwards and of conv7's data gradient add 32-bit lane offsets: a shape they cannot address runs the WIDE twin
    if constexpr (!WIDE && (x3h_slim_fwd<BN, G, UNPOOL, EPI, NP, WN>() || x3h_slim_dg128<BN, G, UNPOOL, EPI, NP, WN>())) {
        if (!x3h_lane_offsets_fit(p.g.Cout)) return launch_conv_x3h<BN, G, UNPOOL, EPI, NP, WN, true>(p, Te, Fe, s);
    }
    constexpr int SMEM = NP * (8 * G + 2) * XH_HF * X3_ROWB + 3 * NP * BN * 64;
    constexpr int THREADS = (2 * WN * G + 4) * 64;
    static int attr = set_smem(conv3x3_x3h_kernel<BN, G, UNPOOL, EPI, NP, WN, WIDE>, SMEM);
    if (attr) return attr;
    static const int per_cu = (THREADS <= 512 && SMEM <= 80 * 1024) ? 2 : 1;     // 12-wave workgroups never share a CU
    static const int ncu = device_cu_count();
    p.dbg = 0;
#ifdef MTL_X3_PROF
    p.prof = g_x3_prof;
#endif
    p.ntf = (Fe + 15) / 16;
    p.ntt = (Te + 8 * G - 1) / (8 * G);
    p.tiles = p.ntf * p.ntt * p.g.B * p.ntile;
    if (p.tiles <= 0) return MTL_OK;                           // empty extent (a pooled forward with T < 2 or F < 2): no output, no launch
    const int grid = p.tiles < ncu * per_cu ? p.tiles : ncu * per_cu;
    hipLaunchKernelGGL((conv3x3_x3h_kernel<BN, G, UNPOOL, EPI, NP, WN, WIDE>), dim3(grid), dim3(THREADS), SMEM, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

static_assert(EPI_RELU == NARROW_RELU && EPI_POOL == NARROW_POOL && EPI_DGRAD == NARROW_DGRAD, "one numbering of the epilogues");

template <bool UNPOOL, int EPI, int NP>
int dispatch_conv_x3(ConvX3P& p, int Te, int Fe, hipStream_t s) {
    if constexpr (NP == 3) {      // the 32-channel shapes of the large_cnn front-end: mtl_conv_narrow.hip (exact split only)
        if (narrow_conv_serves(p.g.Cin, p.g.Cout, UNPOOL, EPI))
            return narrow_conv_launch(s, NarrowConvP{p.x, p.am_in, p.w3, p.bias, p.act, p.y, p.am_out, p.g.B, p.g.T, p.g.F, p.g.Cin, p.g.Cout,
                                                     p.g.Tp, p.g.Fp, Te, Fe, p.Bt, p.sW, p.sBias, p.widths, p.wshift, 0, 0}, UNPOOL, EPI);
    }
    if (p.g.Cin % 64 || p.g.Cout % 64) return MTL_EINVAL;     // C_in % 64: even number of K-tiles (producer loop is unrolled by 2)
    // 8 x 16 tiles (G = 1: 79 KiB of LDS at BN = 64, two workgroups per CU) measured faster only on the 64 -> 64 layer
    // (conv2 fwd 0.52 -> 0.50 ms, dgrad 0.61 -> 0.59); every 128-wide shape and conv5-dgrad is faster with 16 x 16 tiles.
    if (p.g.Cout % 128 == 0) {
        p.ntile = p.g.Cout / 128;
        return launch_conv_x3h<128, 2, UNPOOL, EPI, NP>(p, Te, Fe, s);
    }
    p.ntile = p.g.Cout / 64;
    // two-piece fp16, 64 output channels: 16 x 16 tiles with FOUR consumer waves of 64 px x 64 ch, two workgroups per CU (LDS-bound with
    // 32-channel waves, see the kernel's header).  Forward: conv2 0.385 -> 0.341 ms.  Data gradients (8-task launches): conv2's (un-pooling
    // source, 64 reduction channels) 2.93 -> 2.46 ms, conv5's (dense, 128) 1.33 -> 1.24 ms, both bit for bit what the 32-channel waves
    // gave; their gated epilogue fits the 128 registers of this shape in the SLIM form of the kernel (before: spills, 0.45 -> 0.71 ms).
    // 8 x 16 tiles with two 64 x 64 waves (G = 1, WN = 1) measured 3.47 ms on conv2's.  The other two classes keep their routes (not measured).
    // The forwards' epilogue in the SLIM form as well (x3h_slim_fwd; before: 144 / 160 bytes of scratch): conv2 + pool 2.21 -> 2.09 ms per
    // 8-task launch, without pool 2.64 -> 2.36, bit for bit.
    if constexpr (NP == 2 && EPI != EPI_DGRAD) return launch_conv_x3h<64, 2, UNPOOL, EPI, NP, 1>(p, Te, Fe, s);
    if constexpr (NP == 2 && UNPOOL && X3H_DG2 != 0) {         // (the SLIM halo fetch addresses a pooled sample with 32-bit byte offsets)
        if (p.g.Cin == 64 && (long)p.g.Tp * p.g.Fp * p.g.Cin < (1L << 30)) return launch_conv_x3h<64, 2, UNPOOL, EPI, NP, 1>(p, Te, Fe, s);
    }
    if constexpr (NP == 2 && !UNPOOL && X3H_DG5 != 0) {
        if (p.g.Cin != 64) return launch_conv_x3h<64, 2, UNPOOL, EPI, NP, 1>(p, Te, Fe, s);
    }
    if (p.g.Cin == 64) return launch_conv_x3h<64, 1, UNPOOL, EPI, NP>(p, Te, Fe, s);
    return launch_conv_x3h<64, 2, UNPOOL, EPI, NP>(p, Te, Fe, s);
}

// ------------------------------------------------------------------ weight gradient
// dW[tap][cin][cout] = sum over valid output pixels of x[t+kw-1, f+kh-1, cin] * dy[t, f, cout]
// GEMM view: M = 9*Cin (64-row tiles never straddle a tap), N = Cout, K = pixels (f fastest), split over grid.z.
struct WgradGeom {
    int B, T, F;    // activation extent
    int Ty, Fy;     // extent over which dy can be non-zero (2*Tp, 2*Fp for pooled layers, else T, F)
    int Tp, Fp;
    int Cin, Cout;
    long npix;      // B*Ty*Fy
    long per_split; // pixels per split (multiple of BK)
};

// pixel cursor: (b, t, f) of a flattened pixel index over the Ty x Fy extent, advanced by BK per K-tile without divisions
struct PixCursor {
    int b, t, f;
    __device__ __forceinline__ void set(long pix, int Ty, int Fy) {
        const int plane = Ty * Fy;
        b = (int)(pix / plane);
        const int rem = (int)(pix - (long)b * plane);
        t = rem / Fy;
        f = rem - t * Fy;
    }
    __device__ __forceinline__ void advance(int n, int Ty, int Fy) {
        f += n;
        while (f >= Fy) {   // at most one iteration for the real layer shapes (Fy >= 80 > BK)
            f -= Fy;
            if (++t >= Ty) {
                t = 0;
                ++b;
            }
        }
    }
};

template <int ROWS>
struct LoadWgradX {  // A: rows = ROWS consecutive (tap, cin) indices, MN-major; a thread's 4 channels never straddle a tap
    using Lds = LdsMN<ROWS>;
    static constexpr int VPR = ROWS / 4, KPP = NT / VPR, NV = BK / KPP;
    struct Regs {
        float4 v[NV];
        unsigned m[NV];
    };
    const float* x;
    WgradGeom g;
    int dt, df, cofs, m4, k0;
    bool row_ok;
    long pbeg, pend;
    PixCursor cur[NV];
    __device__ void init(const float* x_, const WgradGeom& g_, int m0, long pbeg_, long pend_, int tid) {
        x = x_;
        g = g_;
        m4 = (tid % VPR) * 4;
        k0 = tid / VPR;
        const int m = m0 + m4;
        row_ok = m < 9 * g.Cin;
        const int tap = row_ok ? m / g.Cin : 0;
        cofs = row_ok ? m - tap * g.Cin : 0;
        const int kh = tap / 3, kw = tap - kh * 3;
        dt = kw - 1;
        df = kh - 1;
        pbeg = pbeg_;
        pend = pend_;
#pragma unroll
        for (int i = 0; i < NV; ++i) cur[i].set(min(pbeg + k0 + i * KPP, g.npix - 1), g.Ty, g.Fy);
    }
    __device__ __forceinline__ void fetch(int kt, Regs& r, int) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const long pix = pbeg + (long)kt * BK + k0 + i * KPP;
            bool ok = row_ok && pix < pend;
            const int ts = cur[i].t + dt, fs = cur[i].f + df;
            ok = ok && (unsigned)ts < (unsigned)g.T && (unsigned)fs < (unsigned)g.F;
            const int tc = min(max(ts, 0), g.T - 1), fc = min(max(fs, 0), g.F - 1);
            const int bc = min(cur[i].b, g.B - 1);
            r.v[i] = *reinterpret_cast<const float4*>(x + (((long)bc * g.T + tc) * g.F + fc) * g.Cin + cofs);
            r.m[i] = ok ? 15u : 0u;
            cur[i].advance(BK, g.Ty, g.Fy);
        }
    }
    __device__ __forceinline__ void commit(float* lds, const Regs& r, int) const {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            *reinterpret_cast<float4*>(&lds[(k0 + i * KPP) * Lds::LD + m4]) = mask4(r.v[i], r.m[i]);
    }
};

template <int BN, bool UNPOOL>
struct LoadWgradDy {  // B: rows = BN output channels, MN-major; dense dy or (dp, argmax)
    using Lds = LdsMN<BN>;
    static constexpr int VPR = BN / 4, KPP = NT / VPR, NV = BK / KPP;
    struct Regs {
        float4 v[NV];
        uchar4 a[NV];
        unsigned m[NV];
    };
    const float* dy;
    const uint8_t* am;
    WgradGeom g;
    int n0, m4, k0;
    long pbeg, pend;
    PixCursor cur[NV];
    __device__ void init(const float* dy_, const uint8_t* am_, const WgradGeom& g_, int n0_, long pbeg_, long pend_, int tid) {
        dy = dy_;
        am = am_;
        g = g_;
        n0 = n0_;
        m4 = (tid % VPR) * 4;
        k0 = tid / VPR;
        pbeg = pbeg_;
        pend = pend_;
        if (UNPOOL) {
#pragma unroll
            for (int i = 0; i < NV; ++i) cur[i].set(min(pbeg + k0 + i * KPP, g.npix - 1), g.Ty, g.Fy);
        }
    }
    __device__ __forceinline__ void fetch(int kt, Regs& r, int) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const long pix = pbeg + (long)kt * BK + k0 + i * KPP;
            const bool ok = pix < pend;
            if (!UNPOOL) {
                r.v[i] = *reinterpret_cast<const float4*>(dy + (ok ? pix : pbeg) * g.Cout + n0 + m4);  // Ty==T, Fy==F
                r.m[i] = ok ? 1u : 0u;
            } else {
                const int t = cur[i].t, f = cur[i].f, bc = min(cur[i].b, g.B - 1);
                const long o = (((long)bc * g.Tp + (t >> 1)) * g.Fp + (f >> 1)) * g.Cout + n0 + m4;
                r.a[i] = *reinterpret_cast<const uchar4*>(am + o);
                r.v[i] = *reinterpret_cast<const float4*>(dy + o);
                r.m[i] = (ok ? 1u : 0u) | ((unsigned)(((f & 1) << 1) | (t & 1)) << 1);
                cur[i].advance(BK, g.Ty, g.Fy);
            }
        }
    }
    __device__ __forceinline__ void commit(float* lds, const Regs& r, int) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 v = r.v[i];
            const bool ok = r.m[i] & 1u;
            if (!UNPOOL) {
                v = mask4(v, ok ? 15u : 0u);
            } else {
                const unsigned sub = r.m[i] >> 1;
                v.x = (ok && r.a[i].x == sub) ? v.x : 0.f;
                v.y = (ok && r.a[i].y == sub) ? v.y : 0.f;
                v.z = (ok && r.a[i].z == sub) ? v.z : 0.f;
                v.w = (ok && r.a[i].w == sub) ? v.w : 0.f;
            }
            *reinterpret_cast<float4*>(&lds[(k0 + i * KPP) * Lds::LD + m4]) = v;
        }
    }
};

struct EpiPartial {
    float* out;  // [9*Cin][Cout] slab of this split
    int m0, n0, Cout, M;
    __device__ __forceinline__ void store4(int lr, int lc, const float (&v)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (m0 + lr + j < M) out[(long)(m0 + lr + j) * Cout + n0 + lc] = v[j];
    }
};

struct WgradP {
    const float* x;
    const float* dy;
    const uint8_t* am;
    float* partial;
    WgradGeom g;
    int mtiles, ntiles, nsplit;
};

template <int BN, bool UNPOOL>
__global__ __launch_bounds__(NT) void conv3x3_wgrad_kernel(WgradP p) {
    using LA = LoadWgradX<128>;
    using LB = LoadWgradDy<BN, UNPOOL>;
    using E = Engine<128, BN, LA, LB>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    // Block order note: giving all (M,N) tiles of one pixel split the same XCD (L % 8) so they share one L2 was measured
    // and REJECTED: the co-scheduled tiles hammer identical cache lines and wgrad dropped 75 -> 61 TF although FETCH_SIZE
    // fell; the plain (tile-fastest) order below lets the 256 MiB Infinity Cache serve the re-reads instead.
    const int split = blockIdx.z;
    const int m0 = blockIdx.x * 128, n0 = blockIdx.y * BN;
    const long pbeg = (long)split * p.g.per_split;
    long pend = pbeg + p.g.per_split;
    if (pend > p.g.npix) pend = p.g.npix;
    LA la;
    LB lb;
    la.init(p.x, p.g, m0, pbeg, pend, tid);
    lb.init(p.dy, p.am, p.g, n0, pbeg, pend, tid);
    f32x16 acc[E::TM][E::TN];
    E::zero(acc);
    const int nk = pend > pbeg ? (int)((pend - pbeg + BK - 1) / BK) : 0;
    if (nk > 0) E::run(la, lb, nk, smem, acc);
    EpiPartial e{p.partial + (long)split * 9 * p.g.Cin * p.g.Cout, m0, n0, p.g.Cout, 9 * p.g.Cin};
    E::finish(acc, e);
}

// dw_ref[cout][cin][kh][kw] += sum_s partial[s][(tap*Cin + cin)][cout]      (fixed order -> deterministic)
// A workgroup owns 64 consecutive elements; its 16 waves split the slabs (wave w: slabs w, w + 16, ...; every load of a thread is
// independent of the others) and combine through LDS in wave order.  The bias gradient (per-slot sums of dy) rides along as Cout
// extra elements behind the weights.  (One thread per element walking all 256 slabs was a latency chain: 69 us for conv2's 37 MB.)
// blockIdx.y = task (several tasks per weight-gradient launch): its nsplit slabs start at slab task * nsplit, its gradients at + task * sDw / sDb
__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int nsplit,
                                                            int Cin, int Cout, const float* __restrict__ bias_part,
                                                            float* __restrict__ db, long sDw = 0, long sDb = 0) {
    __shared__ float sh[16][64];
    if (blockIdx.y) {
        partial += (long)blockIdx.y * nsplit * 9 * Cin * Cout;
        dw += blockIdx.y * sDw;
        if (bias_part) bias_part += (long)blockIdx.y * nsplit * Cout;
        if (db) db += blockIdx.y * sDb;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int total = 9 * Cin * Cout;
    const int e = blockIdx.x * 64 + lane;
    const bool is_w = e < total, is_b = db && e >= total && e < total + Cout;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (is_w || is_b) {
        const float* src = is_w ? partial + e : bias_part + (e - total);
        const long stride = is_w ? total : Cout;
        int k = w;
        for (; k + 48 < nsplit; k += 64) {
            s0 += src[(long)k * stride];
            s1 += src[(long)(k + 16) * stride];
            s2 += src[(long)(k + 32) * stride];
            s3 += src[(long)(k + 48) * stride];
        }
        for (; k < nsplit; k += 16) s0 += src[(long)k * stride];
    }
    sh[w][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (w == 0 && (is_w || is_b)) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += sh[i][lane];
        if (is_w) {
            const int cout = e % Cout;
            const int mc = e / Cout;  // tap*Cin + cin
            const int tap = mc / Cin, cin = mc - tap * Cin;
            dw[((long)cout * Cin + cin) * 9 + tap] += t;
        } else {
            db[e - total] += t;
        }
    }
}

template <int BN, bool UNPOOL>
int launch_wgrad(const WgradP& p, int nsplit, hipStream_t s) {
    using E = Engine<128, BN, LoadWgradX<128>, LoadWgradDy<BN, UNPOOL>>;
    static int attr = set_smem(conv3x3_wgrad_kernel<BN, UNPOOL>, E::SMEM_BYTES);
    if (attr) return attr;
    WgradP q = p;
    q.mtiles = (9 * p.g.Cin + 127) / 128;
    q.ntiles = p.g.Cout / BN;
    q.nsplit = nsplit;
    dim3 grid(q.mtiles, q.ntiles, nsplit);
    hipLaunchKernelGGL((conv3x3_wgrad_kernel<BN, UNPOOL>), grid, dim3(NT), E::SMEM_BYTES, s, q);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

// ------------------------------------------------------------------ x3 weight gradient
// dW[tap][ci][co] = sum over pixels of x[pixel + tap][ci] * dy[pixel][co]: the reduction runs over PIXELS, so both MFMA
// operands want 8 consecutive pixels of one channel per lane while memory is channel-contiguous.
//   * x: a workgroup owns an 8(T) x 16(F) pixel tile and 64 input channels; producers (4 waves) gather the 10 x 18 halo once
//     for all nine taps, split it into the three bf16 pieces and store it as [piece][ci half][halo pixel][32 ci] (64-byte
//     rows).  Consumers fetch A fragments with ds_read_b64_tr_b16 (each 16-lane group transposes a [4 pixels][16 channels]
//     block; four consecutive halo pixels x 64 B = all 64 banks once, conflict-free without padding), tap = constant offset.
//     The halo is double-buffered per pixel tile (8 k-steps x 54 MFMAs per consumer wave).
//   * dy: every B fragment is used by all nine taps of one k-step and by nothing else, so it needs LDS only for the hand-over:
//     each PRODUCER thread owns one fragment per pair of k-steps (lane = output channel, 8 pixels = 8 coalesced 128-byte row
//     loads two pairs ahead, un-pool + split in registers) and stores it in MFMA register layout into a 24 KiB ring read with
//     ds_read_b128; one barrier per two k-steps.  (Consumers doing this themselves cost 25-30 % of the kernel: ablation.)
//   * 4 consumer waves = (ci half, co half) quadrants of a 64 x 64 channel block, nine 32 x 32 accumulators each (one per
//     tap); larger layers are covered by (Cin/64)(Cout/64) workgroup classes.  Workgroups are persistent and write one
//     slab [9*Cin][Cout] sub-block each; wgrad_reduce_kernel sums the slabs in a fixed order (deterministic).
struct WgradX3P {
    const float* x;
    const float* dy;
    const uint8_t* am;
    float* partial;
    int B, T, F, Ty, Fy, Tp, Fp, Cin, Cout;
    int npairs, npj;      // channel-block pairs, and pairs along Cout
    int ntf, ntt, tiles;  // pixel tiles along F, along T, in total (F fastest)
    int dbg;              // ablation switches of probe builds: 1 no halo staging, 2 no dy loads / splits; 0 in production
    const float* amax_x;  // NP = 2: device scalars >= max|x|, >= max|dy|
    const float* amax_dy;
    float* bias_part;     // optional [slot][Cout]: per-slot sums of dy over the slot's pixels (the bias gradient rides along: the
                          // producers see every dy element exactly once per input-channel block; block 0 keeps the sums)
    // several tasks in one launch (round 5): B / tiles count ONE task; the slots are dealt to the tasks in equal contiguous ranges
    // (slot / (nslots / tasks)), a slot walks the pixel tiles of its task only, task k reads its bounds at amax_* + k sAmax* floats.
    // One launch writes nslots partial slabs in total instead of nslots per task (conv7 at 8 tasks: 38 MB instead of 300 MB).
    int tasks;
    long sAmaxX, sAmaxDy;
};

constexpr int WX_HF = 18, WX_NPIX = 10 * WX_HF;          // halo of an 8 x 16 tile
constexpr int WX_SUB = WX_NPIX * 64;                      // one (piece, ci half) sub-plane in bytes; a halo buffer holds 2 NP of them
constexpr int WX_NVA = (WX_NPIX * 16 + NT - 1) / NT;      // float4 per producer thread and tile

typedef short s16x4 __attribute__((ext_vector_type(4)));

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

// B ring: 2 slots x 2 k-steps x [piece][k half][64 co] 16-byte fragments (2 KiB per piece and k-step), behind the two halo buffers
constexpr int wx_smem(int np) { return 2 * (2 * np * WX_SUB) + 4 * (np * 2 * 64 * 16); }

template <bool UNPOOL, int NP>
__global__ __launch_bounds__(512) void conv3x3_wgrad_x3_kernel(WgradX3P p) {
    constexpr int WX_BUF = 2 * NP * WX_SUB, WX_BSTEP = NP * 2 * 64 * 16, WX_BOFF = 2 * WX_BUF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
    const int tid = threadIdx.x;
    // the channel-block pairs of one pixel-tile sequence (slot) sit 8 workgroups apart in dispatch order, i.e. on the SAME XCD, when the
    // grid allows it: the halo / dy tiles they all read then cross the fabric once per L2 instead of once per pair (PMC, round 3: conv7
    // 2.8x, conv5 1.7x the algorithmic bytes with the pairs of a slot on neighbouring XCDs)
    int pair, slot;
    const int nslots = gridDim.x / p.npairs;
    if (gridDim.x % (8 * p.npairs) == 0) {
        const int jb = blockIdx.x >> 3;
        pair = jb % p.npairs;
        slot = (jb / p.npairs) * 8 + (blockIdx.x & 7);
    } else {
        pair = blockIdx.x % p.npairs;
        slot = blockIdx.x / p.npairs;
    }
    const int cib = (pair / p.npj) * 64, cob = (pair % p.npj) * 64;
    const int spt = nslots / p.tasks, task = slot / spt, ls = slot - task * spt;      // slots per task, this slot's task and rank in it
    if (task >= p.tasks) return;                               // (nslots % tasks left-over slots: the whole workgroup, before any barrier)
    const int my_tiles = (p.tiles - ls + spt - 1) / spt;
    const float* amax_x = p.amax_x ? p.amax_x + task * p.sAmaxX : nullptr;
    const float* amax_dy = p.amax_dy ? p.amax_dy + task * p.sAmaxDy : nullptr;
    const int T = p.T, F = p.F, Cin = p.Cin, Cout = p.Cout;
    const int npairs_k = my_tiles * 4;                         // pairs of k-steps (2 x 16 pixels): the B hand-over granule
    // (sample, t0, f0) of this workgroup's j-th tile; each caller keeps its last answer: the producers ask five times per tile, and
    // the two runtime divisions were as many instructions as the rest of their work
    struct TileCache {
        int j = -1, b = 0, t0 = 0, f0 = 0;
    };
    TileCache tc_halo, tc_dy;
    auto tile_of = [&](TileCache& c, int j, int& b, int& t0, int& f0) {
        if (j != c.j) {
            int id = ls + j * spt;
            const int fx = id % p.ntf;
            id /= p.ntf;
            c.f0 = fx * 16;
            c.t0 = (id % p.ntt) * 8;
            c.b = id / p.ntt + task * p.B;                     // (sample index over all tasks: the tensors are contiguous over the tasks)
            c.j = j;
        }
        b = c.b;
        t0 = c.t0;
        f0 = c.f0;
    };

    if (tid >= NT) {
        // ------------------------------------------------------------------ producers: the x halo AND the dy fragments
        const int ptid = tid - NT;
        const float sx = NP == 2 ? pow2_scale(amax_read(amax_x)) : 1.f, sdy = NP == 2 ? pow2_scale(amax_read(amax_dy)) : 1.f;
        float4 hv[WX_NVA];
        unsigned okbits = 0;
        // per-thread constants of the halo gather: element i = halo pixel (ht_i, hf_i), channels c4_i; for a tile whose halo lies inside the
        // image (wave-uniform) the address is base(tile) + woff[i] and every existing element is valid (see conv3x3_x3h_kernel)
        int woff[WX_NVA];
        unsigned wexist = 0;
#pragma unroll
        for (int i = 0; i < WX_NVA; ++i) {
            const int e = ptid + i * NT;
            const int hp = min(e >> 4, WX_NPIX - 1), c4 = (e & 15) * 4;
            const int ht = hp / WX_HF, hf = hp - ht * WX_HF;
            woff[i] = ((ht - 1) * F + (hf - 1)) * Cin + c4;
            wexist |= ((e >> 4) < WX_NPIX ? 1u : 0u) << i;
        }
        auto fetch = [&](int j) {
            int b, t0, f0;
            tile_of(tc_halo, j, b, t0, f0);
            if (t0 >= 1 && t0 + 8 < T && f0 >= 1 && f0 + 16 < F) {
                const float* base = p.x + (((long)b * T + t0) * F + f0) * Cin + cib;
#pragma unroll
                for (int i = 0; i < WX_NVA; ++i) hv[i] = *reinterpret_cast<const float4*>(base + woff[i]);
                okbits = wexist;
                return;
            }
            okbits = 0;
#pragma unroll
            for (int i = 0; i < WX_NVA; ++i) {
                const int e = ptid + i * NT;
                const int hp = min(e >> 4, WX_NPIX - 1), c4 = (e & 15) * 4;
                const int ht = hp / WX_HF, hf = hp - ht * WX_HF;
                const int ts = t0 + ht - 1, fs = f0 + hf - 1;
                const bool ok = (unsigned)ts < (unsigned)T && (unsigned)fs < (unsigned)F;
                const int tc = min(max(ts, 0), T - 1), fc = min(max(fs, 0), F - 1);
                hv[i] = *reinterpret_cast<const float4*>(p.x + (((long)b * T + tc) * F + fc) * Cin + cib + c4);
                okbits |= (ok ? 1u : 0u) << i;
            }
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int i = 0; i < WX_NVA; ++i) {
                const int e = ptid + i * NT;
                if ((e >> 4) >= WX_NPIX) continue;
                const int hp = e >> 4, c4 = (e & 15) * 4;
                const float4 v = mask4(hv[i], ((okbits >> i) & 1u) ? 15u : 0u);
                uint2 pc[NP];
                split_x4<NP>(v, sx, pc);
                unsigned char* dst = smx + buf * WX_BUF + ((c4 >> 5) * WX_NPIX + hp) * 64 + (c4 & 31) * 2;
#pragma unroll
                for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(dst + 2 * q * WX_SUB) = pc[q];
            }
        };
        // dy: this thread owns ONE B fragment per pair of k-steps -- (k-step parity, k half, output channel) -- i.e. 8 pixels
        // of one channel: 8 coalesced row loads (4 + 4 arg-max bytes when pooled), un-pool, 3-way split, three 16-byte stores
        // in the layout the consumers' ds_read_b128 wants ([piece][k half][co], conflict-free).  Loaded two pairs ahead.
        const int bs = ptid >> 7, bhi = (ptid >> 6) & 1, bco = ptid & 63;
        f32x2 bsum2 = {0.f, 0.f};                              // sum of this thread's dy values (bias gradient of channel cob + bco)
        constexpr int NB = UNPOOL ? 4 : 8;
        float bv[2][NB];
        unsigned ba[2], bok[2];
        auto fetch_b = [&](int pk, float (&v)[NB], unsigned& a, unsigned& okm) {
            const int j = pk >> 2, s = (pk & 3) * 2 + bs;
            int b, t0, f0;
            tile_of(tc_dy, min(j, my_tiles - 1), b, t0, f0);
            const int t = t0 + s, fb = f0 + bhi * 8, co = cob + bco;
            okm = 0;
            a = 0;
            if (!UNPOOL) {
                const int tc = min(t, T - 1);
                const int fs = max(min(fb, F - 8), 0);
                const float* rowp = p.dy + (((long)b * T + tc) * F + fs) * Cout + co;
                const bool rowok = t < p.Ty && j < my_tiles;
                if (fs == fb) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = rowp[(long)k * Cout];
                    okm = rowok ? ((fb + 8 <= p.Fy) ? 0xffu : ((1u << max(p.Fy - fb, 0)) - 1u)) : 0u;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int f = fb + k;
                        v[k] = p.dy[(((long)b * T + tc) * F + min(f, F - 1)) * Cout + co];
                        okm |= ((rowok && f < p.Fy) ? 1u : 0u) << k;
                    }
                }
            } else {
                const int tp = min(t >> 1, p.Tp - 1), fp0 = fb >> 1;
                const bool rowok = t < p.Ty && j < my_tiles;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int fp = fp0 + k;
                    const long o = (((long)b * p.Tp + tp) * p.Fp + min(fp, p.Fp - 1)) * Cout + co;
                    v[k] = p.dy[o];
                    a |= (unsigned)p.am[o] << (8 * k);
                    okm |= ((rowok && fp < p.Fp) ? 1u : 0u) << k;
                }
                okm |= (unsigned)(t & 1) << 8;
            }
        };
        auto commit_b = [&](int pk, const float (&v)[NB], unsigned a, unsigned okm) {
            float val[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!UNPOOL) {
                    val[k] = ((okm >> k) & 1u) ? v[k] : 0.f;
                } else {
                    const unsigned sub = ((unsigned)(k & 1) << 1) | (okm >> 8);
                    val[k] = (((okm >> (k >> 1)) & 1u) && ((a >> (8 * (k >> 1))) & 0xffu) == sub) ? v[k >> 1] : 0.f;
                }
            }
            bsum2 += (f32x2{val[0], val[1]} + f32x2{val[2], val[3]}) + (f32x2{val[4], val[5]} + f32x2{val[6], val[7]});      // v_pk_add_f32
            unsigned q0[NP], q1[NP], q2[NP], q3[NP];
            Split<NP>::x2(val[0], val[1], sdy, q0);
            Split<NP>::x2(val[2], val[3], sdy, q1);
            Split<NP>::x2(val[4], val[5], sdy, q2);
            Split<NP>::x2(val[6], val[7], sdy, q3);
            unsigned char* dst = smx + WX_BOFF + ((pk & 1) * 2 + bs) * WX_BSTEP + (bhi * 64 + bco) * 16;
#pragma unroll
            for (int q = 0; q < NP; ++q) *reinterpret_cast<uint4*>(dst + q * 2 * 64 * 16) = make_uint4(q0[q], q1[q], q2[q], q3[q]);
        };
        if (my_tiles > 0) {
            fetch(0);
            fetch_b(0, bv[0], ba[0], bok[0]);
            fetch_b(1, bv[1], ba[1], bok[1]);
            commit(0);
            commit_b(0, bv[0], ba[0], bok[0]);
            fetch_b(2, bv[0], ba[0], bok[0]);
        }
        if (my_tiles > 1) fetch(1);
        __syncthreads();                                       // halo 0 and the fragments of pair 0 are visible
#pragma unroll 1
        for (int pk = 0; pk < npairs_k; pk += 2) {
            // pair pk is being consumed; write pair pk + 1 (its slot was released by the previous barrier), fetch pair pk + 3
            commit_b(pk + 1, bv[1], ba[1], bok[1]);
            fetch_b(pk + 3, bv[1], ba[1], bok[1]);
            __syncthreads();
            commit_b(pk + 2, bv[0], ba[0], bok[0]);
            fetch_b(pk + 4, bv[0], ba[0], bok[0]);
            if ((pk & 3) == 2) {                               // last pair of tile j: the next tile's halo goes into the other buffer
                const int j = pk >> 2;
                if (j + 1 < my_tiles) {
                    commit((j + 1) & 1);
                    if (j + 2 < my_tiles) fetch(j + 2);
                }
            }
            __syncthreads();
        }
        if (p.bias_part && cib == 0) {      // the four threads of a channel (k-step parity x k half) combine in a fixed order
            float* sb = reinterpret_cast<float*>(smx);           // the halo buffers are free now (all consumers are past the last barrier)
            sb[(bs * 2 + bhi) * 64 + bco] = bsum2.x + bsum2.y;
            __syncthreads();                                      // matched by the consumers' barrier in front of their slab stores
            if (ptid < 64) p.bias_part[(long)slot * Cout + cob + bco] = (sb[bco] + sb[64 + bco]) + (sb[128 + bco] + sb[192 + bco]);
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers: quadrant (qi, qj) of the 64 x 64 block
    const int lane = tid & 63, wave = tid >> 6;
    const int qi = wave >> 1, qj = wave & 1;
    const int g = lane >> 4, x16 = lane & 15, l31 = lane & 31, hi = lane >> 5;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    // halo pixel (s + kw) * 18 + f + kh with f = (g >> 1) * 8 + r * 4 + (x16 >> 2); channels qi * 32 + 16 * (g & 1) + 4 * (x16 & 3)
    const int abase = ((qi * WX_NPIX) + (g >> 1) * 8 + (x16 >> 2)) * 64 + (16 * (g & 1) + 4 * (x16 & 3)) * 2;
    const int co = cob + qj * 32 + l31;
    const unsigned char* Bl = smx + WX_BOFF + (hi * 64 + qj * 32 + l31) * 16;
    __syncthreads();
#pragma unroll 1
    for (int pk = 0; pk < npairs_k; ++pk) {
        const int j = pk >> 2;
        const unsigned char* A = smx + (j & 1) * WX_BUF + abase + (pk & 3) * 2 * WX_HF * 64;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned char* Bs = Bl + ((pk & 1) * 2 + s) * WX_BSTEP;
            uint4 b3[NP];
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) b3[pc] = *reinterpret_cast<const uint4*>(Bs + pc * 2 * 64 * 16);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
                const unsigned char* At = A + ((s + kw) * WX_HF + kh) * 64;
                uint4 a3[NP];
#pragma unroll
                for (int pc = 0; pc < NP; ++pc) a3[pc] = tr_read8(At + 2 * pc * WX_SUB);
                acc[tap] = Split<NP>::mfma(a3, b3, acc[tap]);
            }
        }
        __syncthreads();
    }
    if (p.bias_part && cib == 0) __syncthreads();                  // the producers' bias-gradient hand-over (they use LDS once more)
    float* slab = p.partial + (long)slot * 9 * Cin * Cout;
    const float inv = NP == 2 ? 1.f / (pow2_scale(amax_read(amax_x)) * pow2_scale(amax_read(amax_dy))) : 1.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int ci = cib + qi * 32 + 8 * (v >> 2) + 4 * hi + (v & 3);
            slab[((long)tap * Cin + ci) * Cout + co] = NP == 2 ? acc[tap][v] * inv : acc[tap][v];
        }
}

// ------------------------------------------------------------------ weight gradient of a POOLED layer on the 2:4-sparse matrix cores
// conv2 / conv7 are followed by ReLU + 2x2 max-pool (models/asr/transformer.py:50-52,56-58): the gradient that reaches their output
// lives on the pooled grid, and the un-pooled dy the product dW = sum_px x[px + tap] dy[px] consumes has exactly ONE non-zero per
// pooling window and channel -- 75 % structural zeros that the dense kernel above multiplies anyway.  With the pixels of a window as
// four consecutive reduction indices this is (more than) the 2:4 pattern of v_smfmac_f32_32x32x32_f16: per window the sparse operand
// stores {value, 0} and a 2-bit index = the stored arg-max code, and one instruction covers 32 pixels with the matrix work of 16.
// Register layout of the instruction (measured: tools/probe/smfmac_probe.hip, profiles/r4/smfmac_layout.txt):
//   A (sparse, 8 fp16 per lane): lane = (m = lane & 31, ha = lane >> 5); element pair p = e >> 1 covers the dense reduction indices
//       k = 16 (p >> 1) + 8 ha + 4 (p & 1) + {0..3}, element e picks index bits [2 e + 1 : 2 e] of the lane's own index register;
//   B (dense, 16 fp16 per lane): lane = (n = lane & 31, hb = lane >> 5) holds k = 16 hb + e;  C / D: the usual 32 x 32 layout.
// Here M = output channels (dy, sparse), N = input channels (x), K = pixels: k = 4 * window + position, windows along F inside one
// window row of an 8 x 16 pixel tile (8 windows = one instruction), position = the arg-max code (f & 1) << 1 | (t & 1).
//   * x halo: staged exactly as above ([piece][ci half][halo pixel][32 ci]).  A consumer lane fetches, per time offset kw, the
//     COLUMN STRIP its four windows need for all three frequency offsets: five ds_read_b64_tr_b16 per piece, each returning one
//     column pair x both rows -- a 32-bit register is one halo column (two rows), so the B fragment of frequency offset kh is
//     registers [kh, kh + 8) of the strip: 30 LDS reads per 27 instructions instead of 72 per 54.
//   * dy: a producer thread owns (window row parity, ha, output channel): four pooled values + four arg-max bytes, split into the
//     two fp16 pieces, stored as {v, 0} pairs in instruction layout + the 16 index bits; bias gradient sums ride along as before.
#ifndef MTL_SP_DBG
#define MTL_SP_DBG 0      // ablation builds only (tools/probe): never set in the product build
#endif
constexpr int SP_DBG = MTL_SP_DBG;
constexpr int SP_STEP = 2 * 2 * 64 * 16 + 2 * 64 * 4;             // one window row: [piece][ha][co] 16-byte fragments + [ha][co] index words
constexpr int wsp_smem() { return 2 * (2 * 2 * WX_SUB) + 4 * SP_STEP; }

typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(512) void conv3x3_wgrad_sp_kernel(WgradX3P p) {
    constexpr int NP = 2;
    constexpr int WX_BUF = 2 * NP * WX_SUB, WX_BOFF = 2 * WX_BUF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
    const int tid = threadIdx.x;
    // the channel-block pairs of one pixel-tile sequence (slot) are dispatched 8 workgroups apart, i.e. onto the SAME XCD: the halo and
    // dy tiles they all read are fetched from HBM once per L2 instead of once per pair (conv7: 4 pairs)
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int pair = jb % p.npairs, slot = (jb / p.npairs) * 8 + xcd, nslots = gridDim.x / p.npairs;
    const int cib = (pair / p.npj) * 64, cob = (pair % p.npj) * 64;
    const int spt = nslots / p.tasks, task = slot / spt, ls = slot - task * spt;      // slots per task, this slot's task and rank in it
    if (task >= p.tasks) return;
    const int my_tiles = (p.tiles - ls + spt - 1) / spt;
    const float* amax_x = p.amax_x + task * p.sAmaxX;
    const float* amax_dy = p.amax_dy + task * p.sAmaxDy;
    const int T = p.T, F = p.F, Cin = p.Cin, Cout = p.Cout;
    const int npairs_k = my_tiles * 2;                         // pairs of window rows (2 x 32 pixels): the dy hand-over granule
    struct TileCache {
        int j = -1, b = 0, t0 = 0, f0 = 0;
    };
    TileCache tc_halo, tc_dy;
    auto tile_of = [&](TileCache& c, int j, int& b, int& t0, int& f0) {
        if (j != c.j) {
            int id = ls + j * spt;
            const int fx = id % p.ntf;
            id /= p.ntf;
            c.f0 = fx * 16;
            c.t0 = (id % p.ntt) * 8;
            c.b = id / p.ntt + task * p.B;                     // (sample index over all tasks: the tensors are contiguous over the tasks)
            c.j = j;
        }
        b = c.b;
        t0 = c.t0;
        f0 = c.f0;
    };

    if (tid >= NT) {
        // ------------------------------------------------------------------ producers: the x halo AND the sparse dy fragments
        const int ptid = tid - NT;
        const float sx = pow2_scale(amax_read(amax_x)), sdy = pow2_scale(amax_read(amax_dy));
        float4 hv[WX_NVA];
        unsigned okbits = 0;
        // per-thread constants of the halo gather: element i = halo pixel (ht_i, hf_i), channels c4_i; for a tile whose halo lies inside the
        // image (wave-uniform) the address is base(tile) + woff[i] and every existing element is valid (see conv3x3_x3h_kernel)
        int woff[WX_NVA];
        unsigned wexist = 0;
#pragma unroll
        for (int i = 0; i < WX_NVA; ++i) {
            const int e = ptid + i * NT;
            const int hp = min(e >> 4, WX_NPIX - 1), c4 = (e & 15) * 4;
            const int ht = hp / WX_HF, hf = hp - ht * WX_HF;
            woff[i] = ((ht - 1) * F + (hf - 1)) * Cin + c4;
            wexist |= ((e >> 4) < WX_NPIX ? 1u : 0u) << i;
        }
        // fetch / commit take a HALF of the thread's elements (h = 0: i < WX_NVA / 2, h = 1: the rest): the staging of the next tile's halo
        // is spread over both barrier intervals of the current tile (all of it in the second one made the consumers wait there)
        constexpr int HV2 = WX_NVA / 2;
        auto fetch = [&](int j, int h) {
            int b, t0, f0;
            tile_of(tc_halo, j, b, t0, f0);
            const int i0 = h ? HV2 : 0, i1 = h ? WX_NVA : HV2;
            if (t0 >= 1 && t0 + 8 < T && f0 >= 1 && f0 + 16 < F) {
                const float* base = p.x + (((long)b * T + t0) * F + f0) * Cin + cib;
#pragma unroll
                for (int i = 0; i < WX_NVA; ++i)
                    if (i >= i0 && i < i1) hv[i] = *reinterpret_cast<const float4*>(base + woff[i]);
                const unsigned m = ((1u << i1) - 1u) & ~((1u << i0) - 1u);
                okbits = (okbits & ~m) | (wexist & m);
                return;
            }
#pragma unroll
            for (int i = 0; i < WX_NVA; ++i) {
                if (i < i0 || i >= i1) continue;
                const int e = ptid + i * NT;
                const int hp = min(e >> 4, WX_NPIX - 1), c4 = (e & 15) * 4;
                const int ht = hp / WX_HF, hf = hp - ht * WX_HF;
                const int ts = t0 + ht - 1, fs = f0 + hf - 1;
                const bool ok = (unsigned)ts < (unsigned)T && (unsigned)fs < (unsigned)F;
                const int tc = min(max(ts, 0), T - 1), fc = min(max(fs, 0), F - 1);
                hv[i] = *reinterpret_cast<const float4*>(p.x + (((long)b * T + tc) * F + fc) * Cin + cib + c4);
                okbits = (okbits & ~(1u << i)) | ((ok ? 1u : 0u) << i);
            }
        };
        auto commit = [&](int buf, int h) {
            const int i0 = h ? HV2 : 0, i1 = h ? WX_NVA : HV2;
#pragma unroll
            for (int i = 0; i < WX_NVA; ++i) {
                if (i < i0 || i >= i1) continue;
                const int e = ptid + i * NT;
                if ((e >> 4) >= WX_NPIX) continue;
                const int hp = e >> 4, c4 = (e & 15) * 4;
                const float4 v = mask4(hv[i], ((okbits >> i) & 1u) ? 15u : 0u);
                uint2 pc[NP];
                split_x4<NP>(v, sx, pc);
                unsigned char* dst = smx + buf * WX_BUF + ((c4 >> 5) * WX_NPIX + hp) * 64 + (c4 & 31) * 2;
#pragma unroll
                for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(dst + 2 * q * WX_SUB) = pc[q];
            }
        };
        // dy: this thread owns ONE sparse A fragment per pair of window rows -- (window row parity, ha, output channel): the pooled
        // values of windows {2 ha, 2 ha + 1, 4 + 2 ha, 5 + 2 ha} of that row (the four element pairs of its lane) and their arg-max
        // codes.  Loaded two pairs ahead.
        const int bs = ptid >> 7, bha = (ptid >> 6) & 1, bco = ptid & 63;
        f32x2 bsum2 = {0.f, 0.f};                              // sum of this thread's dy values (bias gradient of channel cob + bco)
        float bv[2][4];
        unsigned ba[2], bok[2];
        auto fetch_b = [&](int pk, float (&v)[4], unsigned& a, unsigned& okm) {
            const int j = pk >> 1, wr = (pk & 1) * 2 + bs;
            int b, t0, f0;
            tile_of(tc_dy, min(j, my_tiles - 1), b, t0, f0);
            const int tp = (t0 >> 1) + wr, co = cob + bco;
            const bool rowok = tp < p.Tp && j < my_tiles;
            okm = 0;
            a = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int fp = (f0 >> 1) + (k >> 1) * 4 + 2 * bha + (k & 1);
                const long o = (((long)b * p.Tp + min(tp, p.Tp - 1)) * p.Fp + min(fp, p.Fp - 1)) * Cout + co;
                v[k] = p.dy[o];
                a |= ((unsigned)p.am[o] & 3u) << (4 * k);       // element 2 k of the lane: index bits [4 k + 1 : 4 k]
                okm |= ((rowok && fp < p.Fp) ? 1u : 0u) << k;
            }
        };
        auto commit_b = [&](int pk, const float (&v)[4], unsigned a, unsigned okm) {
            float val[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = ((okm >> k) & 1u) ? v[k] : 0.f;
            bsum2 += f32x2{val[0], val[1]} + f32x2{val[2], val[3]};
            unsigned q0[NP], q1[NP];
            Split<NP>::x2(val[0], val[1], sdy, q0);              // packed pairs [piece]: low half = first value
            Split<NP>::x2(val[2], val[3], sdy, q1);
            unsigned char* dst = smx + WX_BOFF + ((pk & 1) * 2 + bs) * SP_STEP;
#pragma unroll
            for (int q = 0; q < NP; ++q)                         // {v, 0} pairs: the value is element 2 k, element 2 k + 1 is zero
                *reinterpret_cast<uint4*>(dst + ((q * 2 + bha) * 64 + bco) * 16) =
                    make_uint4(q0[q] & 0xffffu, q0[q] >> 16, q1[q] & 0xffffu, q1[q] >> 16);
            *reinterpret_cast<unsigned*>(dst + 4 * 64 * 16 + (bha * 64 + bco) * 4) = a;
        };
        constexpr bool dbgF = SP_DBG & 4, dbgC = SP_DBG & 8, dbgB = SP_DBG & 16;      // ablation builds (-DMTL_SP_DBG=..): no halo loads / no halo commit / no dy work
        if (my_tiles > 0) {
            fetch(0, 0);
            fetch(0, 1);
            fetch_b(0, bv[0], ba[0], bok[0]);
            fetch_b(1, bv[1], ba[1], bok[1]);
            commit(0, 0);
            commit(0, 1);
            commit_b(0, bv[0], ba[0], bok[0]);
            fetch_b(2, bv[0], ba[0], bok[0]);
        }
        if (my_tiles > 1) {
            fetch(1, 0);
            fetch(1, 1);
        }
        __syncthreads();                                       // halo 0 and the fragments of pair 0 are visible
#pragma unroll 1
        for (int pk = 0; pk < npairs_k; pk += 2) {             // one tile (two pairs of window rows) per iteration
            const int j = pk >> 1;                             // buffer (j + 1) & 1 was last read during tile j - 1: it is free for all of tile j
            if (!dbgB) {
                commit_b(pk + 1, bv[1], ba[1], bok[1]);
                fetch_b(pk + 3, bv[1], ba[1], bok[1]);
            }
            if (j + 1 < my_tiles) {
                if (!dbgC) commit((j + 1) & 1, 0);
                if (j + 2 < my_tiles && !dbgF) fetch(j + 2, 0);
            }
            __syncthreads();
            if (!dbgB) {
                commit_b(pk + 2, bv[0], ba[0], bok[0]);
                fetch_b(pk + 4, bv[0], ba[0], bok[0]);
            }
            if (j + 1 < my_tiles) {
                if (!dbgC) commit((j + 1) & 1, 1);
                if (j + 2 < my_tiles && !dbgF) fetch(j + 2, 1);
            }
            __syncthreads();
        }
        if (p.bias_part && cib == 0) {      // the four threads of a channel (window row parity x ha) combine in a fixed order
            float* sb = reinterpret_cast<float*>(smx);
            sb[(bs * 2 + bha) * 64 + bco] = bsum2.x + bsum2.y;
            __syncthreads();
            if (ptid < 64) p.bias_part[(long)slot * Cout + cob + bco] = (sb[bco] + sb[64 + bco]) + (sb[128 + bco] + sb[192 + bco]);
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers: quadrant (qo: co half, qc: ci half) of the 64 x 64 block
    const int lane = tid & 63, wave = tid >> 6;
    const int qc = wave >> 1, qo = wave & 1;
    const int g = lane >> 4, x16 = lane & 15, l31 = lane & 31, hi = lane >> 5;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    // this lane's address inside a 16-lane transpose group: row r = x16 >> 2 of the four it fetches = window position (t & 1 = r & 1,
    // f & 1 = r >> 1), channels 16 (g & 1) + 4 (x16 & 3) of the wave's ci half; halo columns start at 8 hi
    const int r = x16 >> 2;
    const int xbase = ((qc * WX_NPIX) + (r & 1) * WX_HF + 8 * hi + (r >> 1)) * 64 + (16 * (g & 1) + 4 * (x16 & 3)) * 2;
    const unsigned char* Al = smx + WX_BOFF + (hi * 64 + qo * 32 + l31) * 16;
    const unsigned char* Il = smx + WX_BOFF + 4 * 64 * 16 + (hi * 64 + qo * 32 + l31) * 4;
    __syncthreads();
#pragma unroll 1
    for (int pk = 0; pk < npairs_k; ++pk) {
        const int j = pk >> 1;
        const unsigned char* X = smx + (j & 1) * WX_BUF + xbase;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int slot_b = ((pk & 1) * 2 + s) * SP_STEP;
            const f16x8 a_h = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(Al + slot_b));
            const f16x8 a_l = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(Al + slot_b + 2 * 64 * 16));
            const int idx = (int)*reinterpret_cast<const unsigned*>(Il + slot_b);
            const int wr = (pk & 1) * 2 + s;                   // window row inside the tile: halo rows 2 wr + kw, + 1
            // strips are double-buffered by hand: the reads of time offset kw + 1 are issued before the nine instructions of kw (pinned
            // with sched_barrier: left alone, hipcc hoists all 50 strip reads of a pair above the first instruction and spills the
            // accumulators: 337 VGPRs spilled)
            unsigned strip[2][NP][10];                         // [buffer][piece][halo column 8 hi + i]
            auto load_strip = [&](unsigned (&st)[NP][10], int kw) {
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        const s16x4 q = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (__attribute__((address_space(3))) s16x4*)(X + 2 * pc * WX_SUB + ((2 * wr + kw) * WX_HF + 2 * c) * 64));
                        const uint2 u = __builtin_bit_cast(uint2, q);
                        st[pc][2 * c] = u.x;
                        st[pc][2 * c + 1] = u.y;
                    }
            };
            if (SP_DBG & 2) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc)
#pragma unroll
                        for (int c = 0; c < 10; ++c) strip[q][pc][c] = 0x3c003c00u + c;
            }
            if (!(SP_DBG & 2)) load_strip(strip[0], 0);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                if (kw + 1 < 3 && !(SP_DBG & 2)) load_strip(strip[(kw + 1) & 1], kw + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    union {
                        unsigned u[8];
                        f16x16 v;
                    } bh, bl;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        bh.u[i] = strip[kw & 1][0][kh + i];
                        bl.u[i] = strip[kw & 1][1][kh + i];
                    }
                    f32x16 cc = acc[kh * 3 + kw];
                    if (SP_DBG & 1) {                                  // ablation: no matrix instructions
                        acc[kh * 3 + kw][0] += __builtin_bit_cast(float, bh.u[0] ^ bl.u[7]);
                        continue;
                    }
                    cc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(a_l, bh.v, cc, idx, 0, 0);     // smallest terms first
                    cc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(a_h, bl.v, cc, idx, 0, 0);
                    acc[kh * 3 + kw] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(a_h, bh.v, cc, idx, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
    if (p.bias_part && cib == 0) __syncthreads();                  // the producers' bias-gradient hand-over (they use LDS once more)
    float* slab = p.partial + (long)slot * 9 * Cin * Cout;
    const float inv = 1.f / (pow2_scale(amax_read(amax_x)) * pow2_scale(amax_read(amax_dy)));
    const int ci = cib + qc * 32 + l31;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {                           // rows (output channels) 8 v4 + 4 hi + {0..3}: one 16-byte store
            const int co = cob + qo * 32 + 8 * v4 + 4 * hi;
            *reinterpret_cast<float4*>(slab + ((long)tap * Cin + ci) * Cout + co) =
                make_float4(acc[tap][4 * v4] * inv, acc[tap][4 * v4 + 1] * inv, acc[tap][4 * v4 + 2] * inv, acc[tap][4 * v4 + 3] * inv);
        }
}

// w_ref (Cout,Cin,3,3) -> w_fwd[tap][cin][cout]  and  w_dgrad[tap'][cout][cin] with tap' the 180-degree flipped tap
__global__ void conv_wprep_kernel(const float* w, float* wf, float* wd, int Cout, int Cin) {
    const int total = 9 * Cin * Cout;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int tap = e % 9;
        const int cin = (e / 9) % Cin;
        const int cout = e / (9 * Cin);
        const float v = w[e];
        wf[((long)tap * Cin + cin) * Cout + cout] = v;
        wd[((long)(8 - tap) * Cout + cout) * Cin + cin] = v;
    }
}

}  // namespace

// ================================================================== C ABI
// mtl_gemm_f32 with a bias stride for the inner batch index too and a third, outermost batch level (library-internal:
// mtl_gemm_f32_tb forwards here)
int mtl_gemm_f32_3l(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda, const float* B,
                    int ldb, float* C, int ldc, const float* bias, const float* gate, int ldg, int flags, int batch, int H, long sAb,
                    long sAh, long sBb, long sBh, long sCb, long sCh, long sBias, long sBiasH, float* workspace, long workspace_bytes,
                    int tasks, long sAt, long sBt, long sCt, long sBiasT) {
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || H <= 0 || tasks <= 0 || batch % tasks || !A || !B || !C) return MTL_EINVAL;
    GemmP p{A, B, C, bias, gate, M, N, K, lda, ldb, ldc, ldg, alpha, flags, H, sAb, sAh, sBb, sBh, sCb, sCh, 1, 0, nullptr, sBias, sBiasH, batch,
            batch / tasks, sAt, sBt, sCt, sBiasT};
    hipStream_t s = as_stream(stream);
    if (!transA && transB) return dispatch_gemm<false, true>(p, batch, s, workspace, workspace_bytes);
    if (!transA && !transB) return dispatch_gemm<false, false>(p, batch, s, workspace, workspace_bytes);
    if (transA && !transB) return dispatch_gemm<true, false>(p, batch, s, workspace, workspace_bytes);
    return dispatch_gemm<true, true>(p, batch, s, workspace, workspace_bytes);
}

extern "C" {

int mtl_gemm_f32(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                 const float* B, int ldb, float* C, int ldc, const float* bias, const float* gate, int ldg, int flags,
                 int batch, int H, long sAb, long sAh, long sBb, long sBh, long sCb, long sCh, long sBias, float* workspace,
                 long workspace_bytes) {
    return mtl_gemm_f32_3l(stream, transA, transB, M, N, K, alpha, A, lda, B, ldb, C, ldc, bias, gate, ldg, flags, batch, H, sAb, sAh, sBb,
                           sBh, sCb, sCh, sBias, 0, workspace, workspace_bytes, 1, 0, 0, 0, 0);
}

int mtl_conv3x3_wprep(void* stream, const float* w_ref, float* w_fwd, float* w_dgrad, int Cout, int Cin) {
    if (!w_ref || !w_fwd || !w_dgrad) return MTL_EINVAL;
    hipLaunchKernelGGL(conv_wprep_kernel, dim3(grid_for(9L * Cin * Cout, 256)), dim3(256), 0, as_stream(stream), w_ref,
                       w_fwd, w_dgrad, Cout, Cin);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_conv3x3_relu_fwd(void* stream, const float* x, const float* w_fwd, const float* bias, float* y, int B, int T,
                         int F, int Cin, int Cout) {
    if (!x || !w_fwd || !bias || !y) return MTL_EINVAL;
    ConvP p{x, nullptr, w_fwd, bias, nullptr, y, nullptr, {B, T, F, Cin, Cout, T / 2, F / 2}, 1};
    return dispatch_conv<false, EPI_RELU>(p, T, F, as_stream(stream));
}

int mtl_conv3x3_relu_pool_fwd(void* stream, const float* x, const float* w_fwd, const float* bias, float* p_out,
                              unsigned char* argmax, int B, int T, int F, int Cin, int Cout) {
    if (!x || !w_fwd || !bias || !p_out || !argmax) return MTL_EINVAL;
    ConvP p{x, nullptr, w_fwd, bias, nullptr, p_out, argmax, {B, T, F, Cin, Cout, T / 2, F / 2}, 1};
    return dispatch_conv<false, EPI_POOL>(p, 2 * (T / 2), 2 * (F / 2), as_stream(stream));
}

int mtl_conv3x3_dgrad(void* stream, const float* dy, const unsigned char* argmax, const float* w_dgrad,
                      const float* act, float* dx, int B, int T, int F, int Cin, int Cout) {
    // Cin/Cout are the FORWARD conv's channel counts: dy has Cout channels, dx has Cin.
    if (!dy || !w_dgrad || !act || !dx) return MTL_EINVAL;
    ConvP p{dy, argmax, w_dgrad, nullptr, act, dx, nullptr, {B, T, F, Cout, Cin, T / 2, F / 2}, 1};
    if (argmax) return dispatch_conv<true, EPI_DGRAD>(p, T, F, as_stream(stream));
    return dispatch_conv<false, EPI_DGRAD>(p, T, F, as_stream(stream));
}

}  // extern "C"

static int wprep_pieces(int np, hipStream_t s, const float* w_ref, void* wf, void* wd, int Cout, int Cin) {
    if (!w_ref || !wf || !wd || Cin % 32 || Cout % 32) return MTL_EINVAL;
    const long total = 9L * Cin * Cout;
    unsigned short* f = reinterpret_cast<unsigned short*>(wf);
    unsigned short* d = reinterpret_cast<unsigned short*>(wd);
    if (np == 2) {
        hipLaunchKernelGGL(conv_wscale_kernel, dim3(WSCALE_PARTS), dim3(256), 0, s, w_ref, (int)total, reinterpret_cast<float*>(f + 2 * total));
        hipLaunchKernelGGL(conv_wprep_x3_kernel<2>, dim3(grid_for(total, 256)), dim3(256), 0, s, w_ref, f, d, Cout, Cin);
    } else {
        hipLaunchKernelGGL(conv_wprep_x3_kernel<3>, dim3(grid_for(total, 256)), dim3(256), 0, s, w_ref, f, d, Cout, Cin);
    }
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

// the same two kernels for up to three layers at once (grid.y = layer): the pass prepares conv2 / conv5 / conv7 together
struct WprepBatch {
    const float* w[3];
    unsigned short* wf[3];
    unsigned short* wd[3];
    int Cout[3], Cin[3];
    long sSrc, sDst[3];      // parameter set blockIdx.z (the theta' stack): weights at + z sSrc floats, prepared blocks at + z sDst[L] BYTES
};
__global__ __launch_bounds__(256) void conv_wscale_batch_kernel(WprepBatch b) {
    __shared__ float sh[4];
    const int L = blockIdx.y, total = 9 * b.Cin[L] * b.Cout[L];
    b.w[L] += blockIdx.z * b.sSrc;
    b.wf[L] = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(b.wf[L]) + blockIdx.z * b.sDst[L]);
    const float* w = b.w[L];
    float mx = 0.f;
    for (int e = (blockIdx.x * 256 + threadIdx.x) * 4; e < total; e += WSCALE_PARTS * 1024) {
        const float4 v = *reinterpret_cast<const float4*>(w + e);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) reinterpret_cast<float*>(b.wf[L] + 2L * total)[1 + blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__global__ void conv_wprep_h2_batch_kernel(WprepBatch b) {
    const int L = blockIdx.y, Cin = b.Cin[L], Cout = b.Cout[L];
    const float* w = b.w[L] + blockIdx.z * b.sSrc;
    unsigned short* wf = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(b.wf[L]) + blockIdx.z * b.sDst[L]);
    unsigned short* wd = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(b.wd[L]) + blockIdx.z * b.sDst[L]);
    const int total = 9 * Cin * Cout;
    const int nkf = 9 * (Cin / 32), nkd = 9 * (Cout / 32);
    float* hf = reinterpret_cast<float*>(wf + 2L * total);
    float mx = 0.f;
#pragma unroll
    for (int i = 1; i <= WSCALE_PARTS; ++i) mx = fmaxf(mx, hf[i]);
    const float s = pow2_scale(mx);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hf[0] = s;
        *reinterpret_cast<float*>(wd + 2L * total) = s;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int tap = e % 9;
        const int cin = (e / 9) % Cin;
        const int cout = e / (9 * Cin);
        unsigned pc[2];
        Split<2>::x2(w[e], 0.f, s, pc);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const unsigned short v = (unsigned short)(pc[p] & 0xffffu);
            wf[(((long)p * nkf + tap * (Cin / 32) + (cin >> 5)) * Cout + cout) * 32 + x3_swz(cin & 31, cout)] = v;
            wd[(((long)p * nkd + (8 - tap) * (Cout / 32) + (cout >> 5)) * Cin + cin) * 32 + x3_swz(cout & 31, cin)] = v;
        }
    }
}

// tasks of one launch: `tasks` groups of B samples, per-task strides of the prepared weights (bytes), the bias, the input / output bounds (floats)
struct ConvTasks {
    int tasks;
    long sW, sBias, sAmaxIn, sAmaxOut;
    const int* widths = nullptr;
    int wshift = 0;
};
static inline void set_tasks(ConvX3P& p, int B, const ConvTasks& tk) {
    p.Bt = B;
    p.widths = tk.widths;
    p.wshift = tk.wshift;
    p.sW = tk.sW;
    p.sBias = tk.sBias;
    p.sAmaxIn = tk.sAmaxIn;
    p.sAmaxOut = tk.sAmaxOut;
}

template <int NP>
static int conv_fwd_pieces(hipStream_t s, const float* x, const float* amax_x, const void* w, const float* bias, float* y,
                           unsigned char* argmax, float* amax_y, bool pool, int B, int T, int F, int Cin, int Cout,
                           ConvTasks tk = ConvTasks{1, 0, 0, 0, 0}) {
    if (!x || !w || !bias || !y || (pool && !argmax) || (NP == 2 && !amax_x) || tk.tasks < 1 || B < 1) return MTL_EINVAL;
    ConvX3P p{x, nullptr, reinterpret_cast<const unsigned char*>(w), bias, nullptr, y, argmax, {B * tk.tasks, T, F, Cin, Cout, T / 2, F / 2}, 1};
    p.amax_in = amax_x;
    p.amax_out = amax_y;
    set_tasks(p, B, tk);
    if (pool) return dispatch_conv_x3<false, EPI_POOL, NP>(p, 2 * (T / 2), 2 * (F / 2), s);
    return dispatch_conv_x3<false, EPI_RELU, NP>(p, T, F, s);
}

// Edge column of a data gradient whose source lives on the pooled grid of an ODD dense width (F = 2 Fp + 1: conv2 at 161 frequency bins).
// The un-pooled gradient is zero in column F - 1 (floor-mode pooling never selects it), so dx[:, :, F - 1, :] receives only the three taps
// that read column F - 2 -- 1 / 16 of a 16-wide pixel-tile column of the matrix kernel, which would spend a whole tile column on it (one of
// eleven at F = 161).  This kernel computes that column on the vector pipe: dx[b, t, F-1, n] = gate . sum_{kw, k} dyU[b, t+kw-1, F-2, k]
// W[tap kw][k][n] with dy in exact fp32 and W re-assembled from its prepared pieces (two fp16 pieces / scale, or three bf16 pieces: the same
// weight values the matrix kernel multiplies with).  A workgroup: EDGE_PIX rows t of one sample, all n.
constexpr int EDGE_PIX = 32;                   // rows t per workgroup (the re-assembled weights are staged once per workgroup)
constexpr int EDGE_C = 64;                     // channels on both sides (conv2: 64 -> 64, the only odd-width pooled layer of the path)
constexpr int EDGE_SMEM = (3 * EDGE_C * EDGE_C + (EDGE_PIX + 2) * EDGE_C) * 4;
template <int NP>
__global__ __launch_bounds__(256) void conv_dgrad_edge_kernel(ConvX3P p) {
    constexpr int N = EDGE_C, K = EDGE_C;
    const int T = p.g.T, F = p.g.F, Tp = p.g.Tp, Fp = p.g.Fp;
    const int b = blockIdx.y, t0 = blockIdx.x * EDGE_PIX, tid = threadIdx.x;
    const int task = b / p.Bt;
    int rows = T;
    if (p.widths) rows = min(T, ((p.widths[task] >> p.wshift) + 7) / 8 * 8);       // as the matrix kernel: whole 8-row tile rows of the task's frames
    if (t0 >= rows) return;
    extern __shared__ __attribute__((aligned(16))) float edge_lds[];
    float* Ws = edge_lds;                                                          // [3 taps][K][N] fp32, re-assembled from the prepared pieces
    float* src = edge_lds + 3 * K * N;                                             // [EDGE_PIX + 2][K]: un-pooled dy at column F - 2
    const unsigned short* w = reinterpret_cast<const unsigned short*>(p.w3 + task * p.sW);
    constexpr int nk = 9 * (K / 32);
    const float inv_sw = NP == 2 ? 1.f / *reinterpret_cast<const float*>(p.w3 + task * p.sW + (long)NP * nk * N * 64) : 1.f;
    // taps kh = 0 (source column f - 1), kw = 0 .. 2 (rows t - 1 .. t + 1): K-tiles kw * (K / 32) + kc; a K-tile row n holds 32 k (16-byte chunks, swizzled)
#pragma unroll 1
    for (int e = tid; e < 3 * (K / 32) * N * 4; e += 256) {
        const int chunk = e & 3, n = (e >> 2) % N, kt = e / (4 * N);                // kt = kw * (K / 32) + kc
        float v[8] = {};
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const uint4 raw = *reinterpret_cast<const uint4*>(w + ((long)q * nk + kt) * N * 32 + n * 32 + chunk * 8);
            const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned short bits = (unsigned short)(u[j >> 1] >> (16 * (j & 1)));
                v[j] += NP == 2 ? (float)__builtin_bit_cast(_Float16, bits) : __builtin_bit_cast(float, (unsigned)bits << 16);
            }
        }
        const int kk0 = ((chunk ^ ((n >> 2) & 3)) << 3);                            // x3_swz: chunk c of row n holds k = 8 (c ^ ((n >> 2) & 3)) ..
        const int kw = kt / (K / 32), kc = kt - kw * (K / 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) Ws[(kw * K + kc * 32 + kk0 + j) * N + n] = v[j] * inv_sw;
    }
    const int fs = F - 2, fp = fs >> 1;
    // gathered per POOLED element, as the halo waves of the matrix kernel do: t0 is even, so rows t0 - 1 .. t0 + EDGE_PIX (r = 0 .. EDGE_PIX + 1)
    // lie in EDGE_PIX / 2 + 2 window rows, row r in window (r + 1) >> 1 at parity (r + 1) & 1; a window row inside Tp has both its rows inside T
    static_assert(EDGE_PIX % 2 == 0, "even row origins");
    for (int e = tid; e < (EDGE_PIX / 2 + 2) * K; e += 256) {
        const int wr = e / K, k = e - wr * K, tp = (t0 >> 1) - 1 + wr;
        float v = 0.f;
        unsigned code = 255u;                                                      // (no window: neither row matches)
        if (tp >= 0 && tp < Tp && fp < Fp) {
            const long o = (((long)b * Tp + tp) * Fp + fp) * K + k;
            v = p.x[o];
            code = p.am_in[o];
        }
        const unsigned sub = (unsigned)((fs & 1) << 1);
        if (wr > 0) src[(2 * wr - 1) * K + k] = code == sub ? v : 0.f;
        if (wr <= EDGE_PIX / 2) src[2 * wr * K + k] = code == (sub | 1u) ? v : 0.f;
    }
    __syncthreads();
    constexpr int PPG = EDGE_PIX / 4;                                              // 4 waves: wave g owns rows [g PPG, (g + 1) PPG), lane = n
    const int n = tid & 63, grp = tid >> 6;
    float acc[PPG] = {};
#pragma unroll 1
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll 2
        for (int k = 0; k < K; k += 4) {
            const float w0 = Ws[(kw * K + k) * N + n], w1 = Ws[(kw * K + k + 1) * N + n], w2 = Ws[(kw * K + k + 2) * N + n],
                        w3 = Ws[(kw * K + k + 3) * N + n];
#pragma unroll
            for (int i = 0; i < PPG; ++i) {
                const float4 sv = *reinterpret_cast<const float4*>(src + (grp * PPG + i + kw) * K + k);      // (wave-uniform address: broadcast)
                acc[i] += sv.x * w0 + sv.y * w1 + sv.z * w2 + sv.w * w3;
            }
        }
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < PPG; ++i) {
        const int t = t0 + grp * PPG + i;
        if (t < rows) {
            const long o = (((long)b * T + t) * F + (F - 1)) * N + n;
            const float v = p.act[o] > 0.f ? acc[i] : 0.f;
            p.y[o] = v;
            mx = fmaxf(mx, fabsf(v));
        }
    }
    if (p.amax_out) amax_raise(p.amax_out + task * p.sAmaxOut, mx);
}

template <int NP>
static int conv_dgrad_pieces(hipStream_t s, const float* dy, const float* amax_dy, const unsigned char* argmax, const void* w,
                             const float* act, float* dx, float* amax_dx, int B, int T, int F, int Cin, int Cout,
                             ConvTasks tk = ConvTasks{1, 0, 0, 0, 0}) {
    if (!dy || !w || !act || !dx || (NP == 2 && !amax_dy) || tk.tasks < 1 || B < 1) return MTL_EINVAL;
    ConvX3P p{dy, argmax, reinterpret_cast<const unsigned char*>(w), nullptr, act, dx, nullptr, {B * tk.tasks, T, F, Cout, Cin, T / 2, F / 2}, 1};
    p.amax_in = amax_dy;
    p.amax_out = amax_dx;
    set_tasks(p, B, tk);
    if (!argmax) return dispatch_conv_x3<false, EPI_DGRAD, NP>(p, T, F, s);
    // odd width under a pooled source: the matrix kernel covers columns [0, F - 1), the last column goes to the edge kernel
#ifndef MTL_DGRAD_EDGE
#define MTL_DGRAD_EDGE 1     // (0: probe builds for A/B runs -- the matrix kernel spends a tile column on the last frequency bin)
#endif
    const bool edge = MTL_DGRAD_EDGE && (F & 1) && F >= 3 && T >= 1 && Cin == EDGE_C && Cout == EDGE_C && B * tk.tasks <= 65535;
    const int rc = dispatch_conv_x3<true, EPI_DGRAD, NP>(p, T, edge ? F - 1 : F, s);
    if (rc != MTL_OK || !edge) return rc;
    static int attr = set_smem(conv_dgrad_edge_kernel<NP>, EDGE_SMEM);
    if (attr) return attr;
    hipLaunchKernelGGL(conv_dgrad_edge_kernel<NP>, dim3((T + EDGE_PIX - 1) / EDGE_PIX, B * tk.tasks), dim3(256), EDGE_SMEM, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

extern "C" {

int mtl_conv3x3_wprep_x3(void* stream, const float* w_ref, void* w3_fwd, void* w3_dgrad, int Cout, int Cin) {
    return wprep_pieces(3, as_stream(stream), w_ref, w3_fwd, w3_dgrad, Cout, Cin);
}

int mtl_conv3x3_relu_fwd_x3(void* stream, const float* x, const void* w3_fwd, const float* bias, float* y, int B, int T, int F,
                            int Cin, int Cout) {
    return conv_fwd_pieces<3>(as_stream(stream), x, nullptr, w3_fwd, bias, y, nullptr, nullptr, false, B, T, F, Cin, Cout);
}

int mtl_conv3x3_relu_pool_fwd_x3(void* stream, const float* x, const void* w3_fwd, const float* bias, float* p_out,
                                 unsigned char* argmax, int B, int T, int F, int Cin, int Cout) {
    return conv_fwd_pieces<3>(as_stream(stream), x, nullptr, w3_fwd, bias, p_out, argmax, nullptr, true, B, T, F, Cin, Cout);
}

int mtl_conv3x3_dgrad_x3(void* stream, const float* dy, const unsigned char* argmax, const void* w3_dgrad, const float* act,
                         float* dx, int B, int T, int F, int Cin, int Cout) {
    return conv_dgrad_pieces<3>(as_stream(stream), dy, nullptr, argmax, w3_dgrad, act, dx, nullptr, B, T, F, Cin, Cout);
}

static int wprep_h2_batch_sets(void* stream, int n, const float* w0, void* f0, void* d0, int Cout0, int Cin0, const float* w1, void* f1,
                               void* d1, int Cout1, int Cin1, const float* w2, void* f2, void* d2, int Cout2, int Cin2, int sets, long sSrc,
                               long sDst0, long sDst1, long sDst2) {
    if (n < 1 || n > 3 || sets < 1 || sets > 65535) return MTL_EINVAL;
    WprepBatch b{{w0, w1, w2},
                 {reinterpret_cast<unsigned short*>(f0), reinterpret_cast<unsigned short*>(f1), reinterpret_cast<unsigned short*>(f2)},
                 {reinterpret_cast<unsigned short*>(d0), reinterpret_cast<unsigned short*>(d1), reinterpret_cast<unsigned short*>(d2)},
                 {Cout0, Cout1, Cout2},
                 {Cin0, Cin1, Cin2},
                 sSrc,
                 {sDst0, sDst1, sDst2}};
    long tmax = 0;
    for (int i = 0; i < n; ++i) {
        if (!b.w[i] || !b.wf[i] || !b.wd[i] || b.Cin[i] % 32 || b.Cout[i] % 32 || b.Cin[i] <= 0 || b.Cout[i] <= 0) return MTL_EINVAL;
        if (sets > 1 && ((b.sDst[i] & 3) || (sSrc & 3))) return MTL_EINVAL;
        const long t = 9L * b.Cin[i] * b.Cout[i];
        tmax = t > tmax ? t : tmax;
    }
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(conv_wscale_batch_kernel, dim3(WSCALE_PARTS, n, sets), dim3(256), 0, s, b);
    hipLaunchKernelGGL(conv_wprep_h2_batch_kernel, dim3(grid_for(tmax, 256, 256), n, sets), dim3(256), 0, s, b);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_conv3x3_wprep_h2_batch(void* stream, int n, const float* w0, void* f0, void* d0, int Cout0, int Cin0, const float* w1, void* f1,
                               void* d1, int Cout1, int Cin1, const float* w2, void* f2, void* d2, int Cout2, int Cin2) {
    return wprep_h2_batch_sets(stream, n, w0, f0, d0, Cout0, Cin0, w1, f1, d1, Cout1, Cin1, w2, f2, d2, Cout2, Cin2, 1, 0, 0, 0, 0);
}

int mtl_conv3x3_wprep_h2_batch_tb(void* stream, int n, const float* w0, void* f0, void* d0, int Cout0, int Cin0, const float* w1, void* f1,
                                  void* d1, int Cout1, int Cin1, const float* w2, void* f2, void* d2, int Cout2, int Cin2, int sets,
                                  long sSrc, long sDst0, long sDst1, long sDst2) {
    return wprep_h2_batch_sets(stream, n, w0, f0, d0, Cout0, Cin0, w1, f1, d1, Cout1, Cin1, w2, f2, d2, Cout2, Cin2, sets, sSrc, sDst0, sDst1,
                               sDst2);
}

long mtl_conv3x3_wprep_h2_bytes(int Cout, int Cin) { return 2L * 9 * Cin * Cout * 2 + 4 * (1 + WSCALE_PARTS) + 12; }

int mtl_conv3x3_wprep_h2(void* stream, const float* w_ref, void* w2_fwd, void* w2_dgrad, int Cout, int Cin) {
    return wprep_pieces(2, as_stream(stream), w_ref, w2_fwd, w2_dgrad, Cout, Cin);
}

int mtl_conv3x3_relu_fwd_h2(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* y,
                            float* amax_y, int B, int T, int F, int Cin, int Cout) {
    return conv_fwd_pieces<2>(as_stream(stream), x, amax_x, w2_fwd, bias, y, nullptr, amax_y, false, B, T, F, Cin, Cout);
}

int mtl_conv3x3_relu_pool_fwd_h2(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias,
                                 float* p_out, unsigned char* argmax, float* amax_p, int B, int T, int F, int Cin, int Cout) {
    return conv_fwd_pieces<2>(as_stream(stream), x, amax_x, w2_fwd, bias, p_out, argmax, amax_p, true, B, T, F, Cin, Cout);
}

int mtl_conv3x3_dgrad_h2(void* stream, const float* dy, const float* amax_dy, const unsigned char* argmax, const void* w2_dgrad,
                         const float* act, float* dx, float* amax_dx, int B, int T, int F, int Cin, int Cout) {
    return conv_dgrad_pieces<2>(as_stream(stream), dy, amax_dy, argmax, w2_dgrad, act, dx, amax_dx, B, T, F, Cin, Cout);
}

int mtl_conv3x3_relu_fwd_h2_tb(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* y,
                               float* amax_y, int B, int T, int F, int Cin, int Cout, int tasks, long sW, long sBias, long sAmaxX, long sAmaxY,
                               const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_fwd_pieces<2>(as_stream(stream), x, amax_x, w2_fwd, bias, y, nullptr, amax_y, false, B, T, F, Cin, Cout,
                              ConvTasks{tasks, sW, sBias, sAmaxX, sAmaxY, widths, wshift});
}

int mtl_conv3x3_relu_pool_fwd_h2_tb(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* p_out,
                                    unsigned char* argmax, float* amax_p, int B, int T, int F, int Cin, int Cout, int tasks, long sW,
                                    long sBias, long sAmaxX, long sAmaxP, const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_fwd_pieces<2>(as_stream(stream), x, amax_x, w2_fwd, bias, p_out, argmax, amax_p, true, B, T, F, Cin, Cout,
                              ConvTasks{tasks, sW, sBias, sAmaxX, sAmaxP, widths, wshift});
}

int mtl_conv3x3_dgrad_h2_tb(void* stream, const float* dy, const float* amax_dy, const unsigned char* argmax, const void* w2_dgrad,
                            const float* act, float* dx, float* amax_dx, int B, int T, int F, int Cin, int Cout, int tasks, long sW,
                            long sAmaxDy, long sAmaxDx, const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_dgrad_pieces<2>(as_stream(stream), dy, amax_dy, argmax, w2_dgrad, act, dx, amax_dx, B, T, F, Cin, Cout,
                                ConvTasks{tasks, sW, 0, sAmaxDy, sAmaxDx, widths, wshift});
}

/* the samples of `tasks` meta-tasks in one launch on the exact 3 x bf16 split: no bounds, otherwise as the *_h2_tb entry points */
int mtl_conv3x3_relu_fwd_x3_tb(void* stream, const float* x, const void* w3_fwd, const float* bias, float* y, int B, int T, int F, int Cin,
                               int Cout, int tasks, long sW, long sBias, const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_fwd_pieces<3>(as_stream(stream), x, nullptr, w3_fwd, bias, y, nullptr, nullptr, false, B, T, F, Cin, Cout,
                              ConvTasks{tasks, sW, sBias, 0, 0, widths, wshift});
}

int mtl_conv3x3_relu_pool_fwd_x3_tb(void* stream, const float* x, const void* w3_fwd, const float* bias, float* p_out, unsigned char* argmax,
                                    int B, int T, int F, int Cin, int Cout, int tasks, long sW, long sBias, const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_fwd_pieces<3>(as_stream(stream), x, nullptr, w3_fwd, bias, p_out, argmax, nullptr, true, B, T, F, Cin, Cout,
                              ConvTasks{tasks, sW, sBias, 0, 0, widths, wshift});
}

int mtl_conv3x3_dgrad_x3_tb(void* stream, const float* dy, const unsigned char* argmax, const void* w3_dgrad, const float* act, float* dx,
                            int B, int T, int F, int Cin, int Cout, int tasks, long sW, const int* widths, int wshift) {
    if (wshift < 0 || wshift > 8) return MTL_EINVAL;
    return conv_dgrad_pieces<3>(as_stream(stream), dy, nullptr, argmax, w3_dgrad, act, dx, nullptr, B, T, F, Cin, Cout,
                                ConvTasks{tasks, sW, 0, 0, 0, widths, wshift});
}

long mtl_conv3x3_wgrad_workspace(int B, int T, int F, int Cin, int Cout, int pooled) {
    const int Ty = pooled ? 2 * (T / 2) : T, Fy = pooled ? 2 * (F / 2) : F;
    const long npix = (long)B * Ty * Fy;
    const int tiles = ((9 * Cin + 127) / 128) * (Cout / (Cout % 128 == 0 ? 128 : 64));
    long nsplit = (1024 + tiles - 1) / tiles;
    const long maxsplit = (npix + 1023) / 1024;
    if (nsplit > maxsplit) nsplit = maxsplit;
    if (nsplit < 1) nsplit = 1;
    return nsplit * 9L * Cin * Cout * 4;
}

int mtl_conv3x3_wgrad(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref,
                      float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout) {
    if (!x || !dy || !dw_ref || !workspace || Cin % 64 || Cout % 64) return MTL_EINVAL;
    const int pooled = argmax != nullptr;
    const long need = mtl_conv3x3_wgrad_workspace(B, T, F, Cin, Cout, pooled);
    if (workspace_bytes < need) return MTL_EINVAL;
    const int nsplit = (int)(need / (9L * Cin * Cout * 4));
    WgradGeom g;
    g.B = B;
    g.T = T;
    g.F = F;
    g.Ty = pooled ? 2 * (T / 2) : T;
    g.Fy = pooled ? 2 * (F / 2) : F;
    g.Tp = T / 2;
    g.Fp = F / 2;
    g.Cin = Cin;
    g.Cout = Cout;
    g.npix = (long)B * g.Ty * g.Fy;
    long per = (g.npix + nsplit - 1) / nsplit;
    g.per_split = (per + BK - 1) / BK * BK;
    WgradP p{x, dy, argmax, workspace, g, 0, 0, 0};
    hipStream_t s = as_stream(stream);
    int rc;
    if (Cout % 128 == 0)
        rc = pooled ? launch_wgrad<128, true>(p, nsplit, s) : launch_wgrad<128, false>(p, nsplit, s);
    else
        rc = pooled ? launch_wgrad<64, true>(p, nsplit, s) : launch_wgrad<64, false>(p, nsplit, s);
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((9 * Cin * Cout + 63) / 64), dim3(1024), 0, s, workspace, dw_ref,
                       nsplit, Cin, Cout, nullptr, nullptr);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

static int wgrad_x3_grid(int Cin, int Cout) {
    const int npairs = (Cin / 64) * (Cout / 64);
    const int ncu = device_cu_count();
    const int grid = ncu / npairs * npairs;
    return grid < npairs ? npairs : grid;
}

long mtl_conv3x3_wgrad_x3_workspace(int B, int T, int F, int Cin, int Cout, int pooled) {
    (void)B;
    (void)T;
    (void)F;
    (void)pooled;
    if (narrow_wgrad_serves(Cin, Cout)) return narrow_wgrad_slots() * (9L * Cin * Cout * 4 + Cout * 4);      // (exact split only)
    if (Cin % 64 || Cout % 64) return 0;
    const int npairs = (Cin / 64) * (Cout / 64);
    const long nslots = wgrad_x3_grid(Cin, Cout) / npairs;
    return nslots * 9L * Cin * Cout * 4 + nslots * Cout * 4;          // slabs + per-slot bias-gradient sums
}

}  // extern "C"

struct WgradTasks {
    int tasks;
    long sAmaxX, sAmaxDy, sDw, sDb;
};

template <int NP>
static int wgrad_pieces(hipStream_t s, const float* x, const float* amax_x, const float* dy, const float* amax_dy,
                        const unsigned char* argmax, float* dw_ref, float* db, float* workspace, long workspace_bytes, int B, int T,
                        int F, int Cin, int Cout, WgradTasks tk = WgradTasks{1, 0, 0, 0, 0}) {
    if constexpr (NP == 3) {      // the 32-channel shapes of the large_cnn front-end: mtl_conv_narrow.hip, one slab per workgroup
        if (narrow_wgrad_serves(Cin, Cout)) {
            const int slots = narrow_wgrad_slots(), pooled = argmax != nullptr;
            if (!x || !dy || !dw_ref || !workspace || B < 1 || tk.tasks < 1 || tk.tasks > slots) return MTL_EINVAL;
            if (workspace_bytes < mtl_conv3x3_wgrad_x3_workspace(B, T, F, Cin, Cout, pooled)) return MTL_EINVAL;
            const int Ty = pooled ? 2 * (T / 2) : T, Fy = pooled ? 2 * (F / 2) : F;
            if (Ty <= 0 || Fy <= 0) return MTL_OK;               // empty extent: dw / db keep their values, no launch
            float* bias_part = db ? workspace + (long)slots * 9L * Cin * Cout : nullptr;
            const int rc = narrow_wgrad_launch(s, NarrowWgradP{x, dy, argmax, workspace, bias_part, B, T, F, Ty, Fy, T / 2, F / 2, Cout, tk.tasks, 0, 0, 0});
            if (rc) return rc;
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((9 * Cin * Cout + (db ? Cout : 0) + 63) / 64, tk.tasks), dim3(1024), 0, s, workspace, dw_ref,
                               slots / tk.tasks, Cin, Cout, bias_part, db, tk.sDw, tk.sDb);
            MTL_CHECK_LAUNCH();
            return MTL_OK;
        }
    }
    if (!x || !dy || !dw_ref || !workspace || Cin % 64 || Cout % 64 || (NP == 2 && (!amax_x || !amax_dy))) return MTL_EINVAL;
    if (tk.tasks < 1 || tk.tasks > wgrad_x3_grid(Cin, Cout) / ((Cin / 64) * (Cout / 64))) return MTL_EINVAL;
    const int pooled = argmax != nullptr;
    if (workspace_bytes < mtl_conv3x3_wgrad_x3_workspace(B, T, F, Cin, Cout, pooled)) return MTL_EINVAL;
    WgradX3P p;
    p.x = x;
    p.dy = dy;
    p.am = argmax;
    p.partial = workspace;
    p.B = B;
    p.T = T;
    p.F = F;
    p.Ty = pooled ? 2 * (T / 2) : T;
    p.Fy = pooled ? 2 * (F / 2) : F;
    p.Tp = T / 2;
    p.Fp = F / 2;
    p.Cin = Cin;
    p.Cout = Cout;
    p.npj = Cout / 64;
    p.npairs = (Cin / 64) * p.npj;
    p.ntf = (p.Fy + 15) / 16;
    p.ntt = (p.Ty + 7) / 8;
    p.tiles = p.ntf * p.ntt * B;
    if (p.tiles <= 0) return MTL_OK;                            // empty extent (pooled, T < 2 or F < 2): dw / db keep their values, no launch
    p.dbg = 0;
    p.amax_x = amax_x;
    p.amax_dy = amax_dy;
    p.tasks = tk.tasks;
    p.sAmaxX = tk.sAmaxX;
    p.sAmaxDy = tk.sAmaxDy;
    const int grid = wgrad_x3_grid(Cin, Cout);
    const int spt = grid / p.npairs / tk.tasks;                 // slabs per task
    const dim3 rgrid((9 * Cin * Cout + (db ? Cout : 0) + 63) / 64, tk.tasks);
    p.bias_part = db ? workspace + (long)(grid / p.npairs) * 9L * Cin * Cout : nullptr;
    constexpr int SMEM = wx_smem(NP);
    if constexpr (NP == 2) {
        // pooled layers: the 2:4-sparse form
        if (pooled && grid % (8 * p.npairs) == 0) {
            static int attr_sp = set_smem(conv3x3_wgrad_sp_kernel, wsp_smem());
            if (attr_sp) return attr_sp;
            hipLaunchKernelGGL(conv3x3_wgrad_sp_kernel, dim3(grid), dim3(512), wsp_smem(), s, p);
            MTL_CHECK_LAUNCH();
            hipLaunchKernelGGL(wgrad_reduce_kernel, rgrid, dim3(1024), 0, s, workspace, dw_ref, spt, Cin, Cout, p.bias_part, db, tk.sDw, tk.sDb);
            MTL_CHECK_LAUNCH();
            return MTL_OK;
        }
    }
    if (pooled) {
        static int attr = set_smem(conv3x3_wgrad_x3_kernel<true, NP>, SMEM);
        if (attr) return attr;
        hipLaunchKernelGGL((conv3x3_wgrad_x3_kernel<true, NP>), dim3(grid), dim3(512), SMEM, s, p);
    } else {
        static int attr = set_smem(conv3x3_wgrad_x3_kernel<false, NP>, SMEM);
        if (attr) return attr;
        hipLaunchKernelGGL((conv3x3_wgrad_x3_kernel<false, NP>), dim3(grid), dim3(512), SMEM, s, p);
    }
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(wgrad_reduce_kernel, rgrid, dim3(1024), 0, s, workspace, dw_ref, spt, Cin, Cout, p.bias_part, db, tk.sDw, tk.sDb);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

extern "C" {

int mtl_conv3x3_wgrad_h2_tb(void* stream, const float* x, const float* amax_x, const float* dy, const float* amax_dy,
                            const unsigned char* argmax, float* dw_ref, float* db, float* workspace, long workspace_bytes, int B, int T,
                            int F, int Cin, int Cout, int tasks, long sAmaxX, long sAmaxDy, long sDw, long sDb) {
    return wgrad_pieces<2>(as_stream(stream), x, amax_x, dy, amax_dy, argmax, dw_ref, db, workspace, workspace_bytes, B, T, F, Cin, Cout,
                           WgradTasks{tasks, sAmaxX, sAmaxDy, sDw, sDb});
}

int mtl_conv3x3_wgrad_x3_tb(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref, float* db,
                            float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout, int tasks, long sDw, long sDb) {
    return wgrad_pieces<3>(as_stream(stream), x, nullptr, dy, nullptr, argmax, dw_ref, db, workspace, workspace_bytes, B, T, F, Cin, Cout,
                           WgradTasks{tasks, 0, 0, sDw, sDb});
}

int mtl_conv3x3_wgrad_x3(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref,
                         float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout) {
    return wgrad_pieces<3>(as_stream(stream), x, nullptr, dy, nullptr, argmax, dw_ref, nullptr, workspace, workspace_bytes, B, T, F, Cin, Cout);
}

int mtl_conv3x3_wgrad_h2(void* stream, const float* x, const float* amax_x, const float* dy, const float* amax_dy,
                         const unsigned char* argmax, float* dw_ref, float* db, float* workspace, long workspace_bytes, int B, int T,
                         int F, int Cin, int Cout) {
    return wgrad_pieces<2>(as_stream(stream), x, amax_x, dy, amax_dy, argmax, dw_ref, db, workspace, workspace_bytes, B, T, F, Cin, Cout);
}

}  // extern "C"
