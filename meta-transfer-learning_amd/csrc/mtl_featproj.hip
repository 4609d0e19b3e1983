// The encoder's input Linear of a model WITHOUT a convolutional front-end (feat_extractor='none'; models/asr/transformer.py:
// the (B, 1, F, T) batch is viewed as (B, F, T), transposed, and modules/encoder.py applies Linear(F -> d) to every frame) on the
// feature planes AS THEY ARRIVE and the weight AS nn.Linear STORES IT:
//   forward   y[(b T + p), n]  = bias[n] + sum_f x[b, f, p] w[n, f]
//   wgrad     dw[n, f]        += sum_{b, p} dy[(b T + p), n] x[b, f, p]
// The activation operand has its contraction index as the SLOW one (a feature row is a contiguous run of frames), the weight's row
// length is F floats (161: neither a multiple of 4 nor 16-byte aligned rows) and T is arbitrary -- no product engine of this library
// takes that, and the route through them needs a transposed + padded copy of every batch and a padded weight per parameter set.
// Here every global access is a dword per lane, coalesced along the operand's contiguous index (frames of x, features of w, outputs
// of dy / y), predicated at the tails: nothing is assumed about alignment and nothing is read past an operand's last element.
//
// Arithmetic: the exact three-bf16-piece split of mtl_gemm_x3.hip (truncating split3), six v_mfma_f32_32x32x16_bf16 per block
// product (smallest cross terms first), fp32 accumulation: fp32-class results.  All reductions run in a fixed order, there are no
// floating-point atomics: two launches on the same inputs give the same bits, and a task's result does not depend on the number of
// tasks in the launch.
//
// LDS image of an operand tile: [piece][row][32 k] bf16 with the 16-byte chunk swizzle of mtl_gemm_x3.hip (chunk c of row r sits
// at c ^ ((r >> 2) & 3): conflict-free ds_read_b128 fragment reads).  One stage; the global loads of tile kt + 1 are in flight
// while tile kt is multiplied.  The forward's floor is the store of y (131 MB at 8 x 8 x 1000 frames x 512), not the matrix pipe.
#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int NT = 256;          // 4 waves
constexpr int BK = 32;           // contraction elements per tile (two MFMA steps of 16)
constexpr int ROWB = 64;         // bytes of one tile row of one piece

__device__ __forceinline__ unsigned pack_hi(float x0, float x1) {      // {bf16 bits of x0 (low half), of x1 (high half)}, truncating
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, x1), __builtin_bit_cast(unsigned, x0), 0x07060302u);
}
// x = h + m + l exactly (mtl_gemm_x3.hip: split3)
__device__ __forceinline__ void split3(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    const float h0 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x0) & 0xffff0000u);
    const float h1 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x1) & 0xffff0000u);
    const float r0 = x0 - h0, r1 = x1 - h1;
    const float m0 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r0) & 0xffff0000u);
    const float m1 = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r1) & 0xffff0000u);
    const float q0 = r0 - m0, q1 = r1 - m1;
    h = pack_hi(x0, x1);
    m = pack_hi(r0, r1);
    l = pack_hi(q0, q1);
}

// byte offset of 16-byte chunk c (8 k) of tile row r inside a piece plane
__device__ __forceinline__ int chunk_at(int r, int c) { return r * ROWB + ((c ^ ((r >> 2) & 3)) << 4); }

// 8 consecutive k of one row -> the row's chunk c in the three piece planes (plane: bytes of one plane)
__device__ __forceinline__ void commit8(unsigned char* lds, int plane, int r, int c, const float (&v)[8]) {
    uint4 pc[3];
    split3(v[0], v[1], pc[0].x, pc[1].x, pc[2].x);
    split3(v[2], v[3], pc[0].y, pc[1].y, pc[2].y);
    split3(v[4], v[5], pc[0].z, pc[1].z, pc[2].z);
    split3(v[6], v[7], pc[0].w, pc[1].w, pc[2].w);
    unsigned char* dst = lds + chunk_at(r, c);
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<uint4*>(dst + q * plane) = pc[q];
}

// the six piece products of one 32 x 32 x 16 block, smallest first (mtl_gemm_x3.hip)
__device__ __forceinline__ void mma6(f32x16& acc, const uint4 (&a)[3], const uint4 (&b)[3]) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int t = 0; t < 6; ++t)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[PA[t]]), __builtin_bit_cast(bf16x8, b[PB[t]]), acc, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------------------------ forward
constexpr int FN = 128;                          // outputs of a workgroup's tile; a wave owns 32 of them for all of the tile's frames
constexpr int F_PLANE_B = FN * ROWB;

struct FwdP {
    const float *x, *w, *bias;
    float* y;
    int B, F, T, N, tilesN;
    long sX, sW, sY;
};

// MB: 32-frame blocks of the tile.  4 (128 frames) wherever a sample has more than 64 frames: the weight tile, which every workgroup
// re-reads and re-splits per K step, then serves twice the output; 2 (64 frames) for short samples
template <int MB>
__global__ __launch_bounds__(NT) void featproj_fwd_kernel(FwdP p) {
    constexpr int FM = 32 * MB, PLANE_A = FM * ROWB, NI = FM / 64, CSTEP = NT / FM;
    __shared__ __attribute__((aligned(16))) unsigned char sm[3 * (PLANE_A + F_PLANE_B)];
    unsigned char* smB = sm + 3 * PLANE_A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int tn = blockIdx.x % p.tilesN, tt = blockIdx.x / p.tilesN;      // output tiles of one frame tile are neighbours: x stays in L2
    const int b = blockIdx.y, task = blockIdx.z;
    const int p0 = tt * FM, n0 = tn * FN;
    const float* xb = p.x + task * p.sX + (long)b * p.F * p.T;
    const float* wt = p.w + task * p.sW;
    // loaders: x -- thread (frame = tid % FM, chunk = tid / FM (+ CSTEP)) fetches 8 features of its frame per chunk (a wave: 64
    // consecutive frames of one feature row per load); w -- thread (row = tid >> 2 (+ 64), chunk = tid & 3) fetches 8 consecutive
    // features of its output row
    const int ap = tid & (FM - 1), ac = tid / FM, pg = p0 + ap;
    const int bc = tid & 3, br = tid >> 2;
    const bool aok = pg < p.T;
    float ra[NI][8], rb[2][8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + (ac + CSTEP * i) * 8 + j;
                ra[i][j] = (aok && k < p.F) ? xb[(long)k * p.T + pg] : 0.f;
            }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + br + 64 * i;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + bc * 8 + j;
                rb[i][j] = (n < p.N && k < p.F) ? wt[(long)n * p.F + k] : 0.f;
            }
        }
    };
    f32x16 acc[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
    const int nk = (p.F + BK - 1) / BK;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int i = 0; i < NI; ++i) commit8(sm, PLANE_A, ap, ac + CSTEP * i, ra[i]);
        commit8(smB, F_PLANE_B, br, bc, rb[0]);
        commit8(smB, F_PLANE_B, br + 64, bc, rb[1]);
        __syncthreads();
        if (kt + 1 < nk) fetch((kt + 1) * BK);          // in flight under the MFMAs
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            uint4 fb[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) fb[q] = *reinterpret_cast<const uint4*>(smB + q * F_PLANE_B + chunk_at(wave * 32 + l31, 2 * st + hi));
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                uint4 fa[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) fa[q] = *reinterpret_cast<const uint4*>(sm + q * PLANE_A + chunk_at(i * 32 + l31, 2 * st + hi));
                mma6(acc[i], fa, fb);
            }
        }
        __syncthreads();
    }
    // accumulator element v of lane (l31, hi): row 8 (v >> 2) + (v & 3) + 4 hi, column l31 of its 32 x 32 block
    const int col = n0 + wave * 32 + l31;
    if (col >= p.N) return;
    const float bb = p.bias ? p.bias[task * p.sW + col] : 0.f;
    float* yb = p.y + task * p.sY + (long)b * p.T * p.N + col;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int fr = p0 + i * 32 + 8 * (v >> 2) + (v & 3) + 4 * hi;
            if (fr < p.T) yb[(long)fr * p.N] = acc[i][v] + bb;
        }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
constexpr int WN = 128;                          // outputs (rows of dw) of a workgroup's tile; a wave owns 32 x (32 NB) features
constexpr int W_PLANE_A = WN * ROWB;
constexpr int SLICE_MIN = 256;                   // rows of the reduction per grid slice at least

struct WgP {
    const float *x, *dy;
    float* ws;
    int B, F, T, N, R, S, Ls, tilesF;
    long sX, sDy;
};

constexpr int wg_nb(int F) { return F <= 64 ? 2 : F <= 128 ? 4 : 6; }       // 32-feature blocks of the tile: it covers F when it can

// the reduction's B T rows in S slices of Ls rows (a multiple of 32): by the row count and the output's tile count alone (never by
// the task count: a task's result is bitwise that of its own launch).  At most 8 slices, or as many as give a task 32 workgroups
// when its output has few tiles (N = r of the factorized stage A: one tile)
__host__ __device__ inline void wg_slices(long R, int F, int N, int* S, int* Ls) {
    const int wf = 32 * wg_nb(F);
    const long tiles = (long)((F + wf - 1) / wf) * ((N + WN - 1) / WN);
    const long cap = tiles >= 4 ? 8 : 32 / tiles;
    long s = (R + SLICE_MIN - 1) / SLICE_MIN;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    const long ls = ((R + s - 1) / s + BK - 1) / BK * BK;
    *Ls = (int)ls;
    *S = (int)((R + ls - 1) / ls);
}

template <int NB>      // 32-feature blocks per tile
__global__ __launch_bounds__(NT) void featproj_wgrad_kernel(WgP p) {
    constexpr int WF = 32 * NB, PLANE_B = WF * ROWB;
    __shared__ __attribute__((aligned(16))) unsigned char sm[3 * (W_PLANE_A + PLANE_B)];
    unsigned char* smB = sm + 3 * W_PLANE_A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int tf = blockIdx.x % p.tilesF, tn = blockIdx.x / p.tilesF;
    const int s = blockIdx.y, task = blockIdx.z;
    const int n0 = tn * WN, f0 = tf * WF;
    const int r_begin = s * p.Ls, r_end = (int)min((long)p.R, (long)r_begin + p.Ls);
    const float* xt = p.x + task * p.sX;
    const float* dyt = p.dy + task * p.sDy;
    // loaders: dy^T -- thread (output = tid & 127, half = tid >> 7) fetches 16 rows of its output column (a wave: 64 consecutive
    // outputs of one row per load); x -- thread (k pair = tid & 15, feature = tid >> 4 (+ 16 ...)) fetches two consecutive rows of
    // 2 NB features (16 lanes: 32 consecutive frames of one feature row, up to a sample boundary)
    const int an = tid & 127, ah = tid >> 7, ng = n0 + an;
    const bool aok = ng < p.N;
    const int kp = tid & 15, fg = tid >> 4;
    float ra[2][8], rb[2 * NB][2];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = r0 + (2 * ah + c) * 8 + j;
                ra[c][j] = (aok && r < r_end) ? dyt[(long)r * p.N + ng] : 0.f;
            }
        const int ra0 = r0 + 2 * kp;                     // rows ra0, ra0 + 1 = (sample, frame) pairs
        const int b0 = ra0 / p.T, q0 = ra0 - b0 * p.T;
        const bool wrap = q0 + 1 == p.T;
        const long o0 = (long)b0 * p.F * p.T + q0, o1 = wrap ? (long)(b0 + 1) * p.F * p.T : o0 + 1;
        const bool ok0 = ra0 < r_end, ok1 = ra0 + 1 < r_end;
#pragma unroll
        for (int i = 0; i < 2 * NB; ++i) {
            const int f = f0 + fg + 16 * i;
            const bool fok = f < p.F;
            const long fo = (long)f * p.T;
            rb[i][0] = (fok && ok0) ? xt[o0 + fo] : 0.f;
            rb[i][1] = (fok && ok1) ? xt[o1 + fo] : 0.f;
        }
    };
    f32x16 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
    const int nk = (r_end - r_begin + BK - 1) / BK;
    if (nk > 0) fetch(r_begin);
    for (int kt = 0; kt < nk; ++kt) {
        commit8(sm, W_PLANE_A, an, 2 * ah, ra[0]);
        commit8(sm, W_PLANE_A, an, 2 * ah + 1, ra[1]);
#pragma unroll
        for (int i = 0; i < 2 * NB; ++i) {
            unsigned pc[3];
            split3(rb[i][0], rb[i][1], pc[0], pc[1], pc[2]);
            const int r = fg + 16 * i;
            unsigned char* dst = smB + chunk_at(r, kp >> 2) + (kp & 3) * 4;
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<unsigned*>(dst + q * PLANE_B) = pc[q];
        }
        __syncthreads();
        if (kt + 1 < nk) fetch(r_begin + (kt + 1) * BK);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            uint4 fa[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) fa[q] = *reinterpret_cast<const uint4*>(sm + q * W_PLANE_A + chunk_at(wave * 32 + l31, 2 * st + hi));
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                uint4 fb[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) fb[q] = *reinterpret_cast<const uint4*>(smB + q * PLANE_B + chunk_at(j * 32 + l31, 2 * st + hi));
                mma6(acc[j], fa, fb);
            }
        }
        __syncthreads();
    }
    float* out = p.ws + ((long)task * p.S + s) * p.N * p.F;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int f = f0 + j * 32 + l31;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = n0 + wave * 32 + 8 * (v >> 2) + (v & 3) + 4 * hi;
            if (f < p.F && n < p.N) out[(long)n * p.F + f] = acc[j][v];
        }
    }
}

// dw_t += the task's S partial slabs, slice 0 first
__global__ __launch_bounds__(256) void featproj_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, long NF, int S, long sG) {
    const int task = blockIdx.y;
    const float* src = ws + (long)task * S * NF;
    float* dst = dw + task * sG;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < NF; i += (long)gridDim.x * 256) {
        float a = src[i];
        for (int q = 1; q < S; ++q) a += src[q * NF + i];
        dst[i] += a;
    }
}

template <int NB>
int launch_wgrad(const WgP& p0, int tasks, hipStream_t s) {
    WgP p = p0;
    p.tilesF = (p.F + 32 * NB - 1) / (32 * NB);
    const long tiles = (long)p.tilesF * ((p.N + WN - 1) / WN);
    if (tiles > 0x7fffffffL) return MTL_EINVAL;
    hipLaunchKernelGGL(featproj_wgrad_kernel<NB>, dim3((unsigned)tiles, p.S, tasks), dim3(NT), 0, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

inline bool dims_ok(int B, int F, int T, int N, int tasks) {
    return B >= 1 && F >= 1 && T >= 1 && N >= 1 && tasks >= 1 && B <= 65535 && tasks <= 65535 && (long)B * T <= 0x7fffffffL - 64 &&
           (long)F * T <= 0x7fffffffL;
}

}  // namespace

/* see include/mtl_hip.h */
extern "C" int mtl_featproj_fwd_tb(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int F, int T, int N,
                                   int tasks, long sX, long sW, long sY) {
    if (!dims_ok(B, F, T, N, tasks) || !x || !w || !y || sX < 0 || sW < 0 || sY < 0) return MTL_EINVAL;
    const int tilesN = (N + FN - 1) / FN, fm = T > 64 ? 128 : 64;
    const long tiles = (long)tilesN * ((T + fm - 1) / fm);
    if (tiles > 0x7fffffffL) return MTL_EINVAL;
    FwdP p{x, w, bias, y, B, F, T, N, tilesN, sX, sW, sY};
    if (fm == 128) hipLaunchKernelGGL(featproj_fwd_kernel<4>, dim3((unsigned)tiles, B, tasks), dim3(NT), 0, as_stream(stream), p);
    else hipLaunchKernelGGL(featproj_fwd_kernel<2>, dim3((unsigned)tiles, B, tasks), dim3(NT), 0, as_stream(stream), p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

extern "C" long mtl_featproj_wgrad_workspace(int B, int F, int T, int N, int tasks) {
    if (!dims_ok(B, F, T, N, tasks)) return MTL_EINVAL;
    int S, Ls;
    wg_slices((long)B * T, F, N, &S, &Ls);
    return (long)tasks * S * N * F * 4;
}

extern "C" int mtl_featproj_wgrad_tb(void* stream, const float* x, const float* dy, float* dw, float* workspace, long workspace_bytes, int B,
                                     int F, int T, int N, int tasks, long sX, long sDy, long sG) {
    if (!dims_ok(B, F, T, N, tasks) || !x || !dy || !dw || !workspace || sX < 0 || sDy < 0 || sG < 0) return MTL_EINVAL;
    if (workspace_bytes < mtl_featproj_wgrad_workspace(B, F, T, N, tasks)) return MTL_EINVAL;
    if (tasks > 1 && sG < (long)N * F) return MTL_EINVAL;       // the tasks' gradients must not overlap
    WgP p{x, dy, workspace, B, F, T, N, B * T, 0, 0, 0, sX, sDy};
    wg_slices(p.R, F, N, &p.S, &p.Ls);
    hipStream_t s = as_stream(stream);
    // the feature tile covers F when it can (dy, the large operand, is then read once): 64, 128 or 192 features
    const int nb = wg_nb(F);
    const int rc = nb == 2 ? launch_wgrad<2>(p, tasks, s) : nb == 4 ? launch_wgrad<4>(p, tasks, s) : launch_wgrad<6>(p, tasks, s);
    if (rc != MTL_OK) return rc;
    const long NF = (long)N * F;
    hipLaunchKernelGGL(featproj_wgrad_sum_kernel, dim3(grid_for(NF, 256, 1024), tasks), dim3(256), 0, s, workspace, dw, NF, p.S, sG);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}
