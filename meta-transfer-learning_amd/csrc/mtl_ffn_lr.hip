// The middle of the factorized feed-forward block (--is-factorized; modules/common_layers.py:134-158) for gfx950 (MI355X) as ONE
// streamed kernel:   h = relu(a . B1^T + b1)   (rows x inner),   c = h . A2^T   (rows x r)
// with a (rows x r) the output of linear_1_a, B1 = linear_1_b.weight (inner x r), b1 its bias, A2 = linear_2_a.weight (r x inner).
//
// As two product calls these are the shapes the tile engines like least: K = r = 100 (four K steps per tile) and then N = r = 100 (a
// quarter of the tile empty), with h written and read back in between.  Together they have the structure of the flash-attention
// forward of csrc/mtl_attn.hip -- a narrow operand against a long streamed axis: a plays the queries with "head size" r, the inner
// units the keys, B1 plays K, A2^T plays V, and bias + ReLU stand where the softmax is.  One workgroup (four waves) owns 64 rows,
// 16 per wave; a wave keeps its 16 x r tile of a as the resident A operand (exact bf16 triples, the contraction padded with zeros
// to a multiple of 32) and streams B1 / b1 / A2 in chunks of 64 inner units through LDS, split into triples on the way.  Per chunk:
//   1. s (16 x 64) = a . B1_chunk^T: the six-MFMA exact split of csrc/mtl_gemm_x3.hip (a0 b0 + a0 b1 + a1 b0 + a1 b1 + a0 b2 + a2 b0,
//      smallest first), four independent accumulators;
//   2. + b1, ReLU, optionally stored (the backward's h1; NULL in forward-only passes);
//   3. C layout -> A layout through a wave-private fp32 LDS patch, split in registers;
//   4. c (16 x r, NT = ceil(r / 16) accumulators that live for the whole loop) += h_chunk . A2_chunk^T, the chunk's share summed on its
//      own first (one rounding of the running sum per chunk).
// Both weight tiles are stored with the contraction along their rows (B1: [unit][k], A2: [j][unit] as in memory), so every B
// fragment is one 16-byte LDS read per piece.  The inner axis is walked in order and nothing is reduced across workgroups: the
// summation order is fixed, results are bitwise reproducible, there are no atomics.  Units beyond `inner` and k beyond r are zeros
// in LDS (relu(0 + 0) = 0 contributes nothing); rows beyond `rows` compute on row rows - 1 and are never stored.
// Fragment conventions: csrc/mtl_attn.hip's header.
#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int FL_ROWS = 64;        // rows per workgroup: 16 per wave
constexpr int FL_CH = 64;          // inner units per chunk
constexpr int FL_LDP = FL_CH + 4;  // floats per row of the wave-private patch
constexpr int FL_RMAX = 128;

struct FfnLrP {
    const float *a, *B1, *b1, *A2;
    float *h, *c;
    int lda, ldc, rows, r, inner;
    long sAt, sWt, sHt, sCt;
};

// exact three-way split of two fp32 values into packed bf16 pairs (csrc/mtl_attn.hip: split3x2)
__device__ __forceinline__ void split3x2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
    const float q0 = r0 - __builtin_bit_cast(float, m << 16), q1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{q0, q1}, bf16x2));
}
struct Frag8 {       // 8 k-values of one operand row as three bf16 pieces
    uint4 p[3];
};
__device__ __forceinline__ Frag8 split8(const float4& x, const float4& y) {
    Frag8 f;
    split3x2(x.x, x.y, f.p[0].x, f.p[1].x, f.p[2].x);
    split3x2(x.z, x.w, f.p[0].y, f.p[1].y, f.p[2].y);
    split3x2(y.x, y.y, f.p[0].z, f.p[1].z, f.p[2].z);
    split3x2(y.z, y.w, f.p[0].w, f.p[1].w, f.p[2].w);
    return f;
}
__device__ __forceinline__ f32x4 x3_mfma(const Frag8& a, const Frag8& b, f32x4 cc) {
    const bf16x8 a0 = __builtin_bit_cast(bf16x8, a.p[0]), a1 = __builtin_bit_cast(bf16x8, a.p[1]), a2 = __builtin_bit_cast(bf16x8, a.p[2]);
    const bf16x8 b0 = __builtin_bit_cast(bf16x8, b.p[0]), b1 = __builtin_bit_cast(bf16x8, b.p[1]), b2 = __builtin_bit_cast(bf16x8, b.p[2]);
    cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, cc, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, cc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, cc, 0, 0, 0);
}
template <int PLANE>
__device__ __forceinline__ Frag8 read_rows(const unsigned char* q) {       // one 16-byte chunk per piece
    Frag8 b;
    b.p[0] = *reinterpret_cast<const uint4*>(q);
    b.p[1] = *reinterpret_cast<const uint4*>(q + PLANE);
    b.p[2] = *reinterpret_cast<const uint4*>(q + 2 * PLANE);
    return b;
}
// (csrc/mtl_attn.hip: wave_lds_sync) this wave's LDS writes before its own later LDS reads
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A ROWS x (32 KSTEPS) fp32 tile of a row-major matrix: HBM -> registers (16-byte loads; rows >= nrows and columns >= ncols read
// as zero; ncols and every offset are multiples of 4, so a load is inside or outside as a whole) -> three bf16 planes in LDS, RS
// bytes per row
template <int ROWS, int KSTEPS>
struct SplitTile {
    static constexpr int VPR = KSTEPS * 8;               // float4 per row
    static constexpr int NV = ROWS * VPR / 256;          // per thread
    static constexpr int RS = KSTEPS * 64 + 16;          // 16 bytes of padding: the fragment reads of 16 rows spread over the banks
    static constexpr int PLANE = ROWS * RS;
    static constexpr int BYTES = 3 * PLANE;
    static_assert(ROWS * VPR % 256 == 0, "tile does not divide among 256 threads");
    float4 v[NV];
    __device__ __forceinline__ void fetch(const float* base, long ld, int row0, int nrows, int col0, int ncols, int tid) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256, row = row0 + idx / VPR, col = col0 + (idx % VPR) * 4;
            const bool ok = row < nrows && col < ncols;
            const float4 x = *reinterpret_cast<const float4*>(base + (ok ? (long)row * ld + col : 0L));
            v[i] = ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ void commit(unsigned char* lds, int tid) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256;
            uint2 h, m, l;
            split3x2(v[i].x, v[i].y, h.x, m.x, l.x);
            split3x2(v[i].z, v[i].w, h.y, m.y, l.y);
            unsigned char* dst = lds + (idx / VPR) * RS + (idx % VPR) * 8;
            *reinterpret_cast<uint2*>(dst) = h;
            *reinterpret_cast<uint2*>(dst + PLANE) = m;
            *reinterpret_cast<uint2*>(dst + 2 * PLANE) = l;
        }
    }
};

// NT = ceil(r / 16): the 16-column accumulators of c; the contraction of the first product runs over KS = ceil(NT / 2) steps of 32
template <int NT>
__global__ __launch_bounds__(256) void ffn_lr_mid_kernel(FfnLrP p) {
    constexpr int KS = (NT + 1) / 2;
    using T1 = SplitTile<FL_CH, KS>;            // B1 chunk: [unit][k]
    using T2 = SplitTile<NT * 16, FL_CH / 32>;  // A2 chunk: [j][unit]
    __shared__ __attribute__((aligned(16))) unsigned char B1s[T1::BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char A2s[T2::BYTES];
    __shared__ __attribute__((aligned(16))) float Ps[4 * 16 * FL_LDP];
    __shared__ float bs[FL_CH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l16 = lane & 15, g = lane >> 4;
    const int task = blockIdx.y, row0 = blockIdx.x * FL_ROWS + 16 * w;
    const int r = p.r, inner = p.inner;
    const float* B1 = p.B1 + task * p.sWt;
    const float* b1 = p.b1 + task * p.sWt;
    const float* A2 = p.A2 + task * p.sWt;
    float* hout = p.h ? p.h + task * p.sHt : nullptr;

    Frag8 af[KS];       // this wave's 16 rows of a, k = 32 s + 8 g + {0..7} of row l16
    {
        const float* arow = p.a + task * p.sAt + (long)min(row0 + l16, p.rows - 1) * p.lda;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k0 = 32 * s + 8 * g;
            const float4 x = k0 < r ? *reinterpret_cast<const float4*>(arow + k0) : z;
            const float4 y = k0 + 4 < r ? *reinterpret_cast<const float4*>(arow + k0 + 4) : z;
            af[s] = split8(x, y);
        }
    }
    f32x4 cacc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) cacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* Pw = Ps + w * 16 * FL_LDP;
    const int nch = (inner + FL_CH - 1) / FL_CH;
    T1 t1;
    T2 t2;
    float bv;
    t1.fetch(B1, r, 0, inner, 0, r, tid);
    t2.fetch(A2, inner, 0, r, 0, inner, tid);
    bv = (tid < FL_CH && tid < inner) ? b1[tid] : 0.f;
    for (int ch = 0; ch < nch; ++ch) {
        const int u0 = ch * FL_CH;
        t1.commit(B1s, tid);
        t2.commit(A2s, tid);
        if (tid < FL_CH) bs[tid] = bv;
        __syncthreads();
        if (ch + 1 < nch) {          // the next chunk's loads fly under this chunk's MFMAs
            t1.fetch(B1, r, u0 + FL_CH, inner, 0, r, tid);
            t2.fetch(A2, inner, 0, r, u0 + FL_CH, inner, tid);
            bv = (tid < FL_CH && u0 + FL_CH + tid < inner) ? b1[u0 + FL_CH + tid] : 0.f;
        }
        // 1. s = a . B1_chunk^T
        f32x4 sc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const unsigned char* src = B1s + l16 * T1::RS + g * 16;
            Frag8 b[2];
            b[0] = read_rows<T1::PLANE>(src);
#pragma unroll
            for (int i = 0; i < KS * 4; ++i) {
                const int s = i >> 2, t = i & 3;
                if (i + 1 < KS * 4) b[(i + 1) & 1] = read_rows<T1::PLANE>(src + ((i + 1) & 3) * 16 * T1::RS + ((i + 1) >> 2) * 64);
                __builtin_amdgcn_sched_barrier(0);
                sc[t] = x3_mfma(af[s], b[i & 1], sc[t]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // 2. bias, ReLU, the optional store; 3. into the patch (C layout: register rr of lane (g, l16) is row 4 g + rr, unit 16 t + l16)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int unit = u0 + 16 * t + l16;
            const float bias = bs[16 * t + l16];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float v = fmaxf(sc[t][rr] + bias, 0.f);
                Pw[(4 * g + rr) * FL_LDP + 16 * t + l16] = v;
                const int row = row0 + 4 * g + rr;
                if (hout && row < p.rows && unit < inner) hout[(long)row * inner + unit] = v;
            }
        }
        wave_lds_sync();
        // 4. c += h_chunk . A2_chunk^T.  The chunk's contribution is formed in an accumulator of its own, from zero, and joins the long-lived
        // one with a single fp32 add: every MFMA rounds its whole accumulator, and six per step on the running sum of the whole inner
        // axis cost twice the two-call route's error at inner = 512; blocked like this the sum is rounded at full size once per chunk
        {
            const float* pa = Pw + l16 * FL_LDP + 8 * g;
            const unsigned char* src = A2s + l16 * T2::RS + g * 16;
            constexpr int S2 = FL_CH / 32;
            Frag8 a[S2];
#pragma unroll
            for (int s = 0; s < S2; ++s) a[s] = split8(*reinterpret_cast<const float4*>(pa + 32 * s), *reinterpret_cast<const float4*>(pa + 32 * s + 4));
            Frag8 b[2];
            b[0] = read_rows<T2::PLANE>(src);
            f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NT * S2; ++i) {
                const int n = i / S2, sidx = i % S2;
                if (i + 1 < NT * S2) b[(i + 1) & 1] = read_rows<T2::PLANE>(src + ((i + 1) / S2) * 16 * T2::RS + ((i + 1) % S2) * 64);
                __builtin_amdgcn_sched_barrier(0);
                part = x3_mfma(a[sidx], b[i & 1], part);
                __builtin_amdgcn_sched_barrier(0);
                if (sidx == S2 - 1) {
                    cacc[n] += part;
                    part = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        __syncthreads();
    }
    float* cout = p.c + task * p.sCt;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = row0 + 4 * g + rr;
        if (row >= p.rows) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = 16 * n + l16;
            if (col < r) cout[(long)row * p.ldc + col] = cacc[n][rr];
        }
    }
}

template <int NT>
void launch(const FfnLrP& p, int tasks, hipStream_t s) {
    hipLaunchKernelGGL((ffn_lr_mid_kernel<NT>), dim3((p.rows + FL_ROWS - 1) / FL_ROWS, tasks), dim3(256), 0, s, p);
}

}  // namespace

extern "C" int mtl_ffn_lr_mid_supported(int r, int inner) {
    return r >= 4 && r <= FL_RMAX && r % 4 == 0 && inner >= 4 && inner % 4 == 0;
}

extern "C" int mtl_ffn_lr_mid_fwd(void* stream, const float* a, int lda, const float* B1, const float* b1, const float* A2, float* h, float* c,
                                  int ldc, int rows, int r, int inner, int tasks, long sAt, long sWt, long sHt, long sCt) {
    if (!mtl_ffn_lr_mid_supported(r, inner) || !a || !B1 || !b1 || !A2 || !c || rows < 1 || tasks < 1 || tasks > 65535) return MTL_EINVAL;
    if (lda < r || ldc < r || lda % 4 || sAt % 4 || sWt % 4) return MTL_EINVAL;                   // 16-byte loads of a / B1 / A2
    if (((uintptr_t)a | (uintptr_t)B1 | (uintptr_t)A2) & 15) return MTL_EINVAL;
    const FfnLrP p = {a, B1, b1, A2, h, c, lda, ldc, rows, r, inner, sAt, sWt, sHt, sCt};
    hipStream_t s = as_stream(stream);
    switch ((r + 15) / 16) {
        case 1: launch<1>(p, tasks, s); break;
        case 2: launch<2>(p, tasks, s); break;
        case 3: launch<3>(p, tasks, s); break;
        case 4: launch<4>(p, tasks, s); break;
        case 5: launch<5>(p, tasks, s); break;
        case 6: launch<6>(p, tasks, s); break;
        case 7: launch<7>(p, tasks, s); break;
        default: launch<8>(p, tasks, s); break;
    }
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}
