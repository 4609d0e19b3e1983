// Persistent LSTM layer kernels for gfx950 (MI355X): all T time steps of one layer in ONE launch per direction.
//
// The LM meta loop (lm/main_meta_transfer.py:277-411 on lm/model/rnn_model.py:12-70: 2-layer nn.LSTM, bptt 35, batch 20) is a chain
// of T dependent steps per layer; as separate launches every step is a 42 MFLOP recurrent product + a cell kernel (280 launches
// per pass at ~12 us each).  Here workgroup w owns the hidden units j in [8 w, 8 w + 8) for the whole sequence:
//   * its 32 rows of W_hh (gate-major: rows g H + j) stay in REGISTERS across the steps -- thread (r = tid & 31, kc = tid >> 5)
//     holds W_hh[row r][kc H/8 .. + H/8) (<= 64 registers);
//   * per step the previous hidden state (B x H, <= 64 KB) is staged in LDS and every thread multiplies its row chunk with the
//     B batch rows (operand reads are LDS broadcasts), the 8 chunk partials of an output are summed in a fixed order, the
//     threads (b, unit) apply the cell (lstm_cell_act, mtl_rnn_cell.h: the per-step lstm_cell_fwd_kernel below calls the same) and
//     store h_t, c_t, the gate activations and the (dropped) copy for the next layer;
//   * a grid-wide hand-off per step: write-through (sc1) stores of the shared payload -> vmcnt(0) -> workgroup barrier -> one lane
//     arrives on a monotonic counter; consumers: one lane polls (relaxed, agent scope), workgroup barrier, sc1 loads.  Every spin
//     is bounded (an error word is set instead of hanging the device); the grid is H / 8 <= 64 workgroups, far below the 256 CUs,
//     so all of them are resident.
// The backward runs the same ownership in reverse time (see lstm_layer_bwd_kernel).  The weight gradients remain three products
// over all T steps (lm.py).  Reductions are fixed-order: bitwise reproducible.
// Shared with mtl_gru.hip: the cell arithmetic and the dropout convention (mtl_rnn_cell.h); the workspace layout, the hand-off, the
// layer backward's row-split partial product, the width dispatch, the launch and the header resets (mtl_handoff.h).
#include "mtl_handoff.h"
#include "mtl_rnn_cell.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct LstmP {
    const float *gx, *whh, *bhh;
    float *hall, *call, *acts, *xout;
    const uint8_t* mask;
    float mscale;
    int T, B, H;
    unsigned* sync;                           // [0] arrivals (zeroed by the launcher), [1] error word
    // backward
    const float* dx_up;
    float* dG;
};

// ------------------------------------------------------------------ LSTM cell (lm/model/rnn_model.py:20 nn.LSTM), one time step
// gates = gx + gh (both B x 4H, biases already added by the two GEMMs), torch order [i | f | g | o]; acts = the activated gates,
// c, h and the optional dropped copy of h for the next layer
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ gh,
                                                            const float* __restrict__ c_prev, float* __restrict__ acts,
                                                            float* __restrict__ c, float* __restrict__ h, float* __restrict__ h_drop,
                                                            const uint8_t* __restrict__ mask, float mscale, int B, int H) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * H) return;
    const int b = e / H, j = e - b * H;
    const long base = (long)b * 4 * H + j;
    const float pre[4] = {gx[base] + gh[base], gx[base + H] + gh[base + H], gx[base + 2 * H] + gh[base + 2 * H],
                          gx[base + 3 * H] + gh[base + 3 * H]};
    const LstmAct a = lstm_cell_act(pre, c_prev[e]);
    acts[base] = a.i;
    acts[base + H] = a.f;
    acts[base + 2 * H] = a.g;
    acts[base + 3 * H] = a.o;
    c[e] = a.c;
    h[e] = a.h;
    if (h_drop) h_drop[e] = dropped(a.h, mask, e, mscale);
}
// dh = dh_up [* mask * mscale] + dh_rec (both nullable), dc_next nullable: dgates = the pre-activation gradients, dc_prev = dc f
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ dh_up, const uint8_t* __restrict__ mask,
                                                            float mscale, const float* __restrict__ dh_rec,
                                                            const float* __restrict__ dc_next, const float* __restrict__ acts,
                                                            const float* __restrict__ c, const float* __restrict__ c_prev,
                                                            float* __restrict__ dgates, float* __restrict__ dc_prev, int B, int H) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * H) return;
    const int b = e / H, j = e - b * H;
    const long base = (long)b * 4 * H + j;
    float dh = dh_up ? dropped(dh_up, mask, e, mscale) : 0.f;
    if (dh_rec) dh += dh_rec[e];
    const LstmGrad d = lstm_cell_grad(dh, dc_next, e, acts[base], acts[base + H], acts[base + 2 * H], acts[base + 3 * H],
                                      c[e], c_prev + e);
    dgates[base] = d.di;
    dgates[base + H] = d.df;
    dgates[base + 2 * H] = d.dg;
    dgates[base + 3 * H] = d.do_;
    dc_prev[e] = d.dc_prev;
}

// ------------------------------------------------------------------------------------------------------------- persistent layer
// B x H floats written by other workgroups -> LDS (same linear layout), 256 threads.  16-byte `sc1` loads issued back to back with ONE
// wait: the relaxed agent-scope atomic loads of HIP (`__hip_atomic_load`) are kept in program order by the compiler -- a wait after every
// load -- which made this copy a chain of 20 memory round trips (5.0 us of a 13.6 us step, measured with s_memrealtime stamps;
// 1.0 us in this form).
__device__ __forceinline__ void stage_shared(float* lds, const float* src, int count, int tid) {
    if (count % 1024 == 0 && count / 1024 <= 16) {
        const int n = count / 1024;
        float4 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < n) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v[k]) : "v"(src + 4 * (tid + 256 * k)) : "memory");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < n) reinterpret_cast<float4*>(lds)[tid + 256 * k] = v[k];
    } else {
        for (int i = tid; i < count / 2; i += 256) {
            float2 v;
            asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(src + 2 * i) : "memory");
            reinterpret_cast<float2*>(lds)[i] = v;
        }
    }
}
// four `sc1` dword loads in flight, one wait (the gate pre-activations of one cell are H floats apart)
__device__ __forceinline__ void load_shared_x4(const float* q, long stride, float (&v)[4]) {
    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(v[0]) : "v"(q) : "memory");
    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(v[1]) : "v"(q + stride) : "memory");
    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(v[2]) : "v"(q + 2 * stride) : "memory");
    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(v[3]) : "v"(q + 3 * stride) : "memory");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int KC>      // H = 8 KC
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void lstm_layer_fwd_kernel(LstmP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int B = p.B, H = 8 * KC, T = p.T;
    float* hs = sm;                     // [B][H]
    float* red = sm + B * H;            // [16 chunks][B][32 rows]
    // thread (rp = tid & 15, kc = tid >> 4): rows 2 rp, 2 rp + 1 of the 32 gate rows x the k chunk [kc H/16, + H/16): every LDS read of
    // the state feeds two rows (half the LDS traffic of one row x H/8 per thread: the product is LDS-bound)
    constexpr int KH = KC / 2;
    const int tid = threadIdx.x, rp = tid & 15, kc = tid >> 4;
    const int j0 = blockIdx.x * LU;
    const unsigned nwg = gridDim.x;
    float w[2][KH];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = 2 * rp + q;
        const float* wrow = p.whh + (long)((r >> 3) * H + j0 + (r & 7)) * H + kc * KH;
#pragma unroll
        for (int i = 0; i < KH; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(wrow + i);
            w[q][i] = v.x, w[q][i + 1] = v.y, w[q][i + 2] = v.z, w[q][i + 3] = v.w;
        }
    }
    const bool cell = tid < B * LU;
    const int cb = tid / LU, cu = tid % LU, cj = j0 + cu;
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    float c_prev = 0.f;
    if (cell) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[g] = p.bhh[g * H + cj];
        c_prev = p.call[(long)cb * H + cj];
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float gxv[4] = {0.f, 0.f, 0.f, 0.f};                    // this step's input contributions: requested before the wait
        if (cell) {
#pragma unroll
            for (int g = 0; g < 4; ++g) gxv[g] = p.gx[((long)t * B + cb) * 4 * H + g * H + cj];
        }
        if (t > 0) grid_wait(p.sync, (unsigned)t * nwg);        // every workgroup has published h_t
        const float* src = p.hall + (long)t * B * H;
        stage_shared(hs, src, B * H, tid);
        __syncthreads();
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const float* hb = hs + b * H + kc * KH;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int i = 0; i < KH; i += 4) {
                const float4 hv = *reinterpret_cast<const float4*>(hb + i);
                a0 = fmaf(w[0][i], hv.x, a0);
                a1 = fmaf(w[1][i], hv.x, a1);
                a0 = fmaf(w[0][i + 1], hv.y, a0);
                a1 = fmaf(w[1][i + 1], hv.y, a1);
                a0 = fmaf(w[0][i + 2], hv.z, a0);
                a1 = fmaf(w[1][i + 2], hv.z, a1);
                a0 = fmaf(w[0][i + 3], hv.w, a0);
                a1 = fmaf(w[1][i + 3], hv.w, a1);
            }
            *reinterpret_cast<float2*>(red + (kc * B + b) * 32 + 2 * rp) = make_float2(a0, a1);
        }
        __syncthreads();
        if (cell) {
            const long row = (long)t * B + cb;
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < NCH; ++q) s += red[(q * B + cb) * 32 + g * 8 + cu];
                pre[g] = gxv[g] + (s + bias[g]);
            }
            const LstmAct a = lstm_cell_act(pre, c_prev);
            float* ac = p.acts + row * 4 * H + cj;
            ac[0] = a.i, ac[H] = a.f, ac[2 * H] = a.g, ac[3 * H] = a.o;
            const long e = row * H + cj;
            p.call[e + (long)B * H] = a.c;             // call[t + 1]
            store_shared(p.hall + e + (long)B * H, a.h);       // hall[t + 1]: read by every workgroup in the next step
            if (p.xout) p.xout[e] = dropped(a.h, p.mask, e, p.mscale);
            c_prev = a.c;
        }
        if (t + 1 < T) grid_arrive(p.sync);
    }
}

// Backward, same ownership as the forward (workgroup w: the 32 gate rows of its 8 units, in registers): the recurrent gradient
// dh_rec_t = dG_{t+1} . W_hh is split by ROWS -- workgroup w multiplies the 32 columns of dG_{t+1} it has just produced itself
// (in LDS) with its 32 rows of W_hh, for all H outputs (thread: 1-2 output units, 32 x 1-2 weights in registers, the dG operand is
// an LDS broadcast) and publishes that partial (B x H, write-through); after the hand-off every workgroup sums the partials of
// its own 8 units over the workgroups in a fixed order.  Per step a workgroup writes B H floats and reads B x 8 x (H / 8) of them
// (the column-split alternative re-reads all of dG_{t+1}, B x 4H, in every workgroup: measured 24 us per step).  Two partial
// buffers alternate with the step parity (a workgroup is at most one hand-off ahead of the slowest).
template <int KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void lstm_layer_bwd_kernel(LstmP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int B = p.B, H = 8 * KC, T = p.T;
    constexpr int JT = KC > 32 ? 2 : 1;           // output units per thread in the partial product
    float* dgs = sm;                              // [B][32]: this workgroup's columns of dG_t (local row = gate * 8 + unit)
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * LU;
    const unsigned nwg = gridDim.x;
    const int jt = tid * JT;                      // first output unit of this thread
    const bool active = jt < H;
    float w[32][JT];
    if (active) load_rowsplit_weights<8 * KC>(w, p.whh, jt);
    float* P = reinterpret_cast<float*>(p.sync) + HDR;        // two buffers of [nwg][B][H] behind the header
    const long pbuf = (long)nwg * B * H;
    const bool cell = tid < B * LU;
    const int cb = tid / LU, cu = tid % LU, cj = j0 + cu;
    float dc_next = 0.f;
#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
        float dh_rec = 0.f;
        // this step's own operands do not depend on the other workgroups: requested before the wait
        float dh_up = 0.f, ai = 0.f, af = 0.f, ag = 0.f, ao = 0.f, cc = 0.f, cprev = 0.f;
        if (cell) {
            const long row = (long)t * B + cb;
            const long e = row * H + cj;
            dh_up = p.dx_up ? dropped(p.dx_up, p.mask, e, p.mscale) : 0.f;
            const float* ac = p.acts + row * 4 * H + cj;
            ai = ac[0], af = ac[H], ag = ac[2 * H], ao = ac[3 * H];
            cc = p.call[e + (long)B * H], cprev = p.call[e];
        }
        if (t < T - 1) {
            grid_wait(p.sync, (unsigned)(T - 1 - t) * nwg);     // every workgroup has published its partial of step t + 1
            if (cell) {
                const float* q = P + ((t + 1) & 1) * pbuf + (long)cb * H + cj;
                float s0 = 0.f, s1 = 0.f;
#pragma unroll 16
                for (unsigned wq = 0; wq < nwg; wq += 2) {      // (32 loads in flight)      // fixed order (nwg = H / 8 is even)
                    s0 += __hip_atomic_load(q + (long)wq * B * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s1 += __hip_atomic_load(q + (long)(wq + 1) * B * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                dh_rec = s0 + s1;
            }
        }
        if (cell) {
            const long row = (long)t * B + cb;
            const LstmGrad d = lstm_cell_grad(dh_up + dh_rec, &dc_next, 0, ai, af, ag, ao, cc, &cprev);
            float* dg = p.dG + row * 4 * H + cj;
            dg[0] = d.di, dg[H] = d.df, dg[2 * H] = d.dg, dg[3 * H] = d.do_;
            float* l = dgs + cb * 32 + cu;
            l[0] = d.di, l[8] = d.df, l[16] = d.dg, l[24] = d.do_;
            dc_next = d.dc_prev;
        }
        if (t > 0) {
            __syncthreads();
            if (active) rowsplit_partial(w, dgs, P + (t & 1) * pbuf + (long)blockIdx.x * B * H + jt, B, H);
            grid_arrive(p.sync);
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Layer stack as ONE wavefront launch per direction: grid = NL x (H / 8) workgroups, workgroup (l, w) owns units [8 w, 8 w + 8) of
// layer l.  Layer l step t needs layer l step t - 1 (its own counter) and layer l - 1 step t (the lower layer's counter), so the
// layers run one step apart instead of one after the other: ~T + NL - 1 hand-offs per pass instead of NL T.
//   forward:  the input contributions W_ih x_t + b_ih of a layer >= 1 are formed per step by a SECOND group of H / 8 workgroups (same
//             ownership, W_ih rows in registers) that depends on the layer below only and therefore runs ahead of its layer: the
//             layer's own step stays as short as layer 0's (inside the layer's workgroups the product cost 8 us of a 20 us step).
//             Layer 0 takes its input contributions from one product over all T steps (gx[0]), as before.
//   backward: layer l >= 1 also multiplies its columns of dG_t with its rows of W_ih: a second row-split partial (the gradient into
//             the lower layer's output) -- computed after the arrival that publishes the recurrent partial, again in the shadow of
//             the hand-off, and acknowledged by the next arrival.  The upper layer is not gated by the lower one and may run ahead,
//             so these partials are buffered for ALL T steps ([NL-1][T][nwg][B][H], p.p2).
struct StackP {
    float* gx[MAXL];
    const float *wih[MAXL], *bih[MAXL], *whh[MAXL], *bhh[MAXL];
    float *hall[MAXL], *call[MAXL], *acts[MAXL], *xout[MAXL], *dG[MAXL];
    const uint8_t* mask[MAXL];
    const float* dx_up;
    float* p2;
    float mscale;
    int T, B, H, NL;
    unsigned* sync;
};

// Hand-off of the stack kernels: every workgroup owns ONE flag word (the number of steps it has published) instead of sharing an
// arrival counter -- 64 read-modify-writes on one address serialise in L2, 64 write-through stores do not; the waiting workgroup's
// first wave reads all flags of a group with one load per poll.
__device__ __forceinline__ void flags_wait(const unsigned* flags, unsigned n, unsigned target, unsigned* err) {
    if (threadIdx.x < 64) {
        unsigned spins = 0;
        for (;;) {
            const unsigned v = threadIdx.x < n ? __hip_atomic_load(flags + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : target;
            if (__all(v >= target)) break;
            if (++spins > SPIN_LIMIT) {
                if (threadIdx.x == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
}
__device__ __forceinline__ void flags_arrive(unsigned* flag, unsigned steps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through stores are acknowledged
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void lstm_stack_fwd_kernel(StackP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int B = p.B, H = 8 * KC, T = p.T, NL = p.NL;
    float* hs = sm;                     // [B][H]: the operand of this group's product (previous state / the lower layer's output)
    float* red = sm + B * H;            // [16 chunks][B][32 rows]
    constexpr int KH = KC / 2;
    const int tid = threadIdx.x, rp = tid & 15, kc = tid >> 4;
    const unsigned nwg = H / LU;
    // groups 0 .. NL-1: the layers; groups NL .. 2 NL - 2: the input products of layers 1 .. NL-1 (they only depend on the layer
    // below, so they run ahead of their layer instead of lengthening its step)
    const int grp = blockIdx.x / nwg, j0 = (blockIdx.x % nwg) * LU;
    const bool xgroup = grp >= NL;
    const int l = xgroup ? grp - NL + 1 : grp;
    const int wg = blockIdx.x % nwg;
    unsigned* own = p.sync + 64 + 64 * l;                    // step flags of layer l
    unsigned* xin = p.sync + 64 + 64 * (MAXL + l);           // step flags of the input-product group of layer l
    unsigned* low = p.sync + 64 + 64 * (l > 0 ? l - 1 : 0);
    unsigned* err = p.sync + 1;
    f32x2 w[KH];      // {row 2 rp, row 2 rp + 1} at column kc KH + i: one packed FMA (v_pk_fma_f32) per column, the state value broadcast
    {
        const float* wsrc = xgroup ? p.wih[l] : p.whh[l];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = 2 * rp + q;
            const float* wrow = wsrc + (long)((r >> 3) * H + j0 + (r & 7)) * H + kc * KH;
#pragma unroll
            for (int i = 0; i < KH; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(wrow + i);
                w[i][q] = v.x, w[i + 1][q] = v.y, w[i + 2][q] = v.z, w[i + 3][q] = v.w;
            }
        }
    }
    const bool cell = tid < B * LU;
    const int cb = tid / LU, cu = tid % LU, cj = j0 + cu;
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    float c_prev = 0.f;
    float* hall = p.hall[l];
    float* call = p.call[l];
    float* acts = p.acts[l];
    float* xout = p.xout[l];
    float* gx = p.gx[l];
    const uint8_t* mask = p.mask[l];
    if (cell) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[g] = (xgroup ? p.bih[l] : p.bhh[l])[g * H + cj];
        if (!xgroup) c_prev = call[(long)cb * H + cj];
    }
    // the B x H operand at `src` (written by other workgroups: sc1 loads) against this thread's two row chunks; the 16 chunk
    // partials of an output are summed in a fixed order by the cell threads (after the barrier)
    auto product = [&](const float* src) {
        stage_shared(hs, src, B * H, tid);
        __syncthreads();
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const float* hb = hs + b * H + kc * KH;
            f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};       // two independent chains (one wave per SIMD: nothing else hides the FMA latency)
#pragma unroll
            for (int i = 0; i < KH; i += 4) {
                const float4 hv = *reinterpret_cast<const float4*>(hb + i);
                a0 = __builtin_elementwise_fma(w[i], f32x2{hv.x, hv.x}, a0);
                a1 = __builtin_elementwise_fma(w[i + 1], f32x2{hv.y, hv.y}, a1);
                a0 = __builtin_elementwise_fma(w[i + 2], f32x2{hv.z, hv.z}, a0);
                a1 = __builtin_elementwise_fma(w[i + 3], f32x2{hv.w, hv.w}, a1);
            }
            *reinterpret_cast<float2*>(red + (kc * B + b) * 32 + 2 * rp) = make_float2(a0.x + a1.x, a0.y + a1.y);
        }
        __syncthreads();
    };
    if (xgroup) {
        const float* xlow = p.xout[l - 1];
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
            flags_wait(low, nwg, (unsigned)(t + 1), err);      // the layer below has published its output of step t
            product(xlow + (long)t * B * H);
            if (cell) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < NCH; ++q) s += red[(q * B + cb) * 32 + g * 8 + cu];
                    store_shared(gx + ((long)t * B + cb) * 4 * H + g * H + cj, s + bias[g]);
                }
            }
            flags_arrive(xin + wg, (unsigned)(t + 1));      // (its barrier also orders the reads of `red` before the next step's writes)
        }
        return;
    }
    // input contributions W_ih x_t + b_ih of this thread's cell.  Layer 0: plain loads issued before the step's wait.  Layers >= 1:
    // written by the input-product group during this launch -- the values of step t + 1 are fetched (after a wait on that group,
    // which runs ahead) at the END of step t, in the shadow of the step's own hand-off, so a step has ONE wait on its critical path
    float gxn[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch_gx = [&](int t) {
        if (l > 0) flags_wait(xin, nwg, (unsigned)(t + 1), err);
        if (cell) {
            const float* q = gx + ((long)t * B + cb) * 4 * H + cj;
            if (l > 0) {
                load_shared_x4(q, H, gxn);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) gxn[g] = q[g * H];
            }
        }
    };
    if (l > 0) fetch_gx(0);
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        if (l == 0) fetch_gx(t);
        float gxv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) gxv[g] = gxn[g];
        if (t > 0) flags_wait(own, nwg, (unsigned)t, err);     // every workgroup of this layer has published h_t
        product(hall + (long)t * B * H);
        if (cell) {
            const long row = (long)t * B + cb;
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < NCH; ++q) s += red[(q * B + cb) * 32 + g * 8 + cu];
                pre[g] = gxv[g] + (s + bias[g]);
            }
            const LstmAct a = lstm_cell_act(pre, c_prev);
            float* ac = acts + row * 4 * H + cj;
            ac[0] = a.i, ac[H] = a.f, ac[2 * H] = a.g, ac[3 * H] = a.o;
            const long e = row * H + cj;
            call[e + (long)B * H] = a.c;
            store_shared(hall + e + (long)B * H, a.h);
            store_shared(xout + e, dropped(a.h, mask, e, p.mscale));      // read by the group above
            c_prev = a.c;
        }
        flags_arrive(own + wg, (unsigned)(t + 1));      // also after the last step: the group above waits for it
        if (l > 0 && t + 1 < T) fetch_gx(t + 1);
    }
}

template <int KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void lstm_stack_bwd_kernel(StackP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int B = p.B, H = 8 * KC, T = p.T, NL = p.NL;
    constexpr int JT = KC > 32 ? 2 : 1;
    float* dgs = sm;                              // [B][32]
    const int tid = threadIdx.x;
    const unsigned nwg = H / LU;
    const int l = blockIdx.x / nwg, wg = blockIdx.x % nwg, j0 = wg * LU;
    unsigned* own = p.sync + 64 + 64 * l;
    unsigned* up = p.sync + 64 + 64 * (l + 1 < NL ? l + 1 : l);
    unsigned* err = p.sync + 1;
    const int jt = tid * JT;
    const bool active = jt < H;
    float w[32][JT], wi[32][JT];
    if (active) {
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const long ro = (long)((r >> 3) * H + j0 + (r & 7)) * H + jt;
#pragma unroll
            for (int c = 0; c < JT; ++c) {
                w[r][c] = p.whh[l][ro + c];
                wi[r][c] = l > 0 ? p.wih[l][ro + c] : 0.f;
            }
        }
    }
    const long pbuf = (long)nwg * B * H;
    float* P1 = reinterpret_cast<float*>(p.sync) + HDR + (long)l * 2 * PBUF;       // this layer's recurrent partials, two parities
    const float* P2r = p.p2 + (long)l * T * pbuf;                                      // partials from the layer above (l < NL - 1)
    float* P2w = l > 0 ? p.p2 + (long)(l - 1) * T * pbuf + (long)wg * B * H : nullptr; // partials for the layer below
    const bool cell = tid < B * LU;
    const int cb = tid / LU, cu = tid % LU, cj = j0 + cu;
    const float* acts = p.acts[l];
    const float* call = p.call[l];
    float* dG = p.dG[l];
    const uint8_t* mask = p.mask[l];
    const bool top = l == NL - 1;
    float dc_next = 0.f;
    // partial product of this workgroup's 32 columns of dG_t (in dgs) with its 32 rows of a weight matrix, all H outputs
    auto partial = [&](const float (&ww)[32][JT], float* out) {
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const float* gb = dgs + b * 32;
            if constexpr (JT == 2) {
                // two output units per thread: one packed FMA (v_pk_fma_f32) per weight pair, the dG operand broadcast to both halves;
                // two accumulator pairs keep the dependent chains at half the length
                f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 32; r += 4) {
                    const float4 gv = *reinterpret_cast<const float4*>(gb + r);
                    a0 = __builtin_elementwise_fma(f32x2{ww[r][0], ww[r][1]}, f32x2{gv.x, gv.x}, a0);
                    a1 = __builtin_elementwise_fma(f32x2{ww[r + 1][0], ww[r + 1][1]}, f32x2{gv.y, gv.y}, a1);
                    a0 = __builtin_elementwise_fma(f32x2{ww[r + 2][0], ww[r + 2][1]}, f32x2{gv.z, gv.z}, a0);
                    a1 = __builtin_elementwise_fma(f32x2{ww[r + 3][0], ww[r + 3][1]}, f32x2{gv.w, gv.w}, a1);
                }
                const float lo = a0.x + a1.x, hi = a0.y + a1.y;
                const unsigned long long u = (unsigned long long)__builtin_bit_cast(unsigned, lo) | ((unsigned long long)__builtin_bit_cast(unsigned, hi) << 32);
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(out + (long)b * H), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int r = 0; r < 32; r += 4) {
                    const float4 gv = *reinterpret_cast<const float4*>(gb + r);
                    a0 = fmaf(gv.x, ww[r][0], a0);
                    a1 = fmaf(gv.y, ww[r + 1][0], a1);
                    a0 = fmaf(gv.z, ww[r + 2][0], a0);
                    a1 = fmaf(gv.w, ww[r + 3][0], a1);
                }
                store_shared(out + (long)b * H, a0 + a1);
            }
        }
    };
    auto gather = [&](const float* q) {            // fixed-order sum of the nwg partials of this thread's (b, unit)
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 32
        for (unsigned wq = 0; wq < nwg; wq += 2) {
            s0 += __hip_atomic_load(q + (long)wq * B * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s1 += __hip_atomic_load(q + (long)(wq + 1) * B * H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return s0 + s1;
    };
    // gradient into this layer's output from the layer above: the sum of its input-gradient partials of step t.  The layer above
    // acknowledges the partial of step t with the arrival of step t - 1 (the final one for t <= 1).
    float dh_up_next = 0.f;
    auto gather_up = [&](int t) {
        const int k = T - t + 1 < T ? T - t + 1 : T;
        flags_wait(up, nwg, (unsigned)k, err);
        if (cell) dh_up_next = gather(P2r + (long)t * pbuf + (long)cb * H + cj);
    };
    if (!top) gather_up(T - 1);
#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
        float dh_rec = 0.f, dh_up = 0.f, ai = 0.f, af = 0.f, ag = 0.f, ao = 0.f, cc = 0.f, cprev = 0.f, keep = 1.f;
        if (cell) {
            const long row = (long)t * B + cb;
            const long e = row * H + cj;
            keep = mask ? (mask[e] ? p.mscale : 0.f) : 1.f;
            if (top) dh_up = p.dx_up[e];
            const float* ac = acts + row * 4 * H + cj;
            ai = ac[0], af = ac[H], ag = ac[2 * H], ao = ac[3 * H];
            cc = call[e + (long)B * H], cprev = call[e];
        }
        if (!top) dh_up = dh_up_next;        // gathered at the end of the previous iteration (below), off this step's critical path
        dh_up *= keep;
        if (t < T - 1) {
            flags_wait(own, nwg, (unsigned)(T - 1 - t), err);
            if (cell) dh_rec = gather(P1 + ((t + 1) & 1) * pbuf + (long)cb * H + cj);
        }
        if (cell) {
            const long row = (long)t * B + cb;
            const float dh = dh_up + dh_rec;
            const LstmGrad d = lstm_cell_grad(dh, &dc_next, 0, ai, af, ag, ao, cc, &cprev);
            float* dg = dG + row * 4 * H + cj;
            dg[0] = d.di, dg[H] = d.df, dg[2 * H] = d.dg, dg[3 * H] = d.do_;
            float* q = dgs + cb * 32 + cu;
            q[0] = d.di, q[8] = d.df, q[16] = d.dg, q[24] = d.do_;
            dc_next = d.dc_prev;
        }
        __syncthreads();
        if (t > 0) {
            if (active) partial(w, P1 + (t & 1) * pbuf + (long)wg * B * H + jt);
            flags_arrive(own + wg, (unsigned)(T - t));
        }
        if (l > 0 && active) partial(wi, P2w + (long)t * pbuf + jt);     // in the shadow of the hand-off; acknowledged by the next arrival
        if (!top && t > 0) gather_up(t - 1);                             // likewise: the next step's input gradient
    }
    if (l > 0) flags_arrive(own + wg, (unsigned)T);
}

// dynamic LDS of lstm_layer_fwd_kernel and lstm_stack_fwd_kernel (one layout): the staged operand [B][H] + the chunk partials
// [NCH][B][32 rows]; the backward kernels hold dG_t [B][32]
constexpr int lstm_fwd_lds(int B, int H) { return (B * H + NCH * B * 32) * 4; }
constexpr int lstm_bwd_lds(int B) { return B * 32 * 4; }

bool fill_stack(StackP& p, const mtl_lstm_stack* d, int NL, bool bwd) {
    for (int l = 0; l < NL; ++l) {
        p.wih[l] = d->w_ih[l], p.bih[l] = d->b_ih[l], p.whh[l] = d->w_hh[l], p.bhh[l] = d->b_hh[l];
        p.hall[l] = d->hall[l], p.call[l] = d->call[l], p.acts[l] = d->acts[l], p.xout[l] = d->xout[l], p.dG[l] = d->dG[l];
        p.mask[l] = d->mask[l], p.gx[l] = d->gx[l];
        if (!p.whh[l] || !p.call[l] || !p.acts[l] || (l > 0 && !p.wih[l])) return false;
        if (bwd ? !p.dG[l] : (!p.bhh[l] || !p.hall[l] || !p.xout[l] || !p.gx[l] || (l > 0 && !p.bih[l]))) return false;
    }
    return true;
}

}  // namespace

extern "C" {

// Every workgroup of a persistent launch must be resident at once (the grid-wide hand-offs spin on each other): the bound is the
// device's own CU count (hipDeviceAttributeMultiprocessorCount: a partitioned / shared device reports its share), minus a margin
// of one eighth for whatever else holds CUs.
static int lstm_resident_limit() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        n = 256;                          // no device visible (shape queries on a build host): the MI355X's own count
    return n - n / 8;
}
int mtl_lstm_cell_fwd(void* stream, const float* gx, const float* gh, const float* c_prev, float* acts, float* c, float* h,
                      float* h_drop, const unsigned char* mask, float mscale, int B, int H) {
    if (!gx || !gh || !c_prev || !acts || !c || !h || B <= 0 || H <= 0) return MTL_EINVAL;
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3((B * H + 255) / 256), dim3(256), 0, as_stream(stream), gx, gh, c_prev, acts, c, h,
                       h_drop, mask, mscale, B, H);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_lstm_cell_bwd(void* stream, const float* dh_up, const unsigned char* mask, float mscale, const float* dh_rec,
                      const float* dc_next, const float* acts, const float* c, const float* c_prev, float* dgates, float* dc_prev,
                      int B, int H) {
    if (!acts || !c || !c_prev || !dgates || !dc_prev || B <= 0 || H <= 0) return MTL_EINVAL;
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((B * H + 255) / 256), dim3(256), 0, as_stream(stream), dh_up, mask, mscale, dh_rec,
                       dc_next, acts, c, c_prev, dgates, dc_prev, B, H);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_lstm_layer_supported(int B, int H) {
    return B >= 1 && B <= MAXB && (H == 128 || H == 256 || H == 384 || H == 512) && H / LU <= lstm_resident_limit();
}

long mtl_lstm_layer_workspace(void) { return HDR * 4 + MAXL * 2 * PBUF * 4; }      // header + two partial buffers per layer (backward)

int mtl_lstm_stack_supported(int B, int H, int NL) {      // every workgroup must be resident: (2 NL - 1) H / 8 of the device's CUs
    return mtl_lstm_layer_supported(B, H) && NL >= 1 && NL <= MAXL && (2 * NL - 1) * (H / LU) <= lstm_resident_limit();
}

long mtl_lstm_stack_scratch(int T, int B, int H, int NL) { return NL > 1 ? (long)(NL - 1) * T * (H / LU) * B * H * 4 : 0; }

int mtl_lstm_stack_fwd(void* stream, const mtl_lstm_stack* layers, float mscale, int T, int B, int H, int NL, void* workspace) {
    if (!layers || !workspace || T <= 0 || !mtl_lstm_stack_supported(B, H, NL)) return MTL_EINVAL;
    StackP p{};
    if (!fill_stack(p, layers, NL, false)) return MTL_EINVAL;
    p.mscale = mscale, p.T = T, p.B = B, p.H = H, p.NL = NL, p.sync = reinterpret_cast<unsigned*>(workspace);
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_flags(workspace, s)) return rc;
    return dispatch_kc(H, [&](auto kc) {
        return launch_persistent<lstm_stack_fwd_kernel<kc()>>((2 * NL - 1) * (H / LU), lstm_fwd_lds(B, H), lstm_fwd_lds(MAXB, H), s, p);
    });
}

int mtl_lstm_stack_bwd(void* stream, const mtl_lstm_stack* layers, const float* dx_up, float mscale, float* scratch, int T, int B, int H,
                       int NL, void* workspace) {
    if (!layers || !dx_up || !workspace || T <= 0 || !mtl_lstm_stack_supported(B, H, NL) || (NL > 1 && !scratch)) return MTL_EINVAL;
    StackP p{};
    if (!fill_stack(p, layers, NL, true)) return MTL_EINVAL;
    p.dx_up = dx_up, p.p2 = scratch, p.mscale = mscale, p.T = T, p.B = B, p.H = H, p.NL = NL, p.sync = reinterpret_cast<unsigned*>(workspace);
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_flags(workspace, s)) return rc;
    return dispatch_kc(H, [&](auto kc) { return launch_persistent<lstm_stack_bwd_kernel<kc()>>(NL * (H / LU), lstm_bwd_lds(B), 0, s, p); });
}

int mtl_lstm_layer_fwd(void* stream, const float* gx, const float* w_hh, const float* b_hh, float* hall, float* call, float* acts,
                       float* xout, const unsigned char* mask, float mscale, int T, int B, int H, void* workspace) {
    if (!gx || !w_hh || !b_hh || !hall || !call || !acts || !workspace || T <= 0 || !mtl_lstm_layer_supported(B, H)) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_counter(workspace, s)) return rc;
    LstmP p{gx, w_hh, b_hh, hall, call, acts, xout, mask, mscale, T, B, H, reinterpret_cast<unsigned*>(workspace), nullptr, nullptr};
    return dispatch_kc(H, [&](auto kc) {
        return launch_persistent<lstm_layer_fwd_kernel<kc()>>(H / LU, lstm_fwd_lds(B, H), lstm_fwd_lds(MAXB, H), s, p);
    });
}

int mtl_lstm_layer_bwd(void* stream, const float* dx_up, const unsigned char* mask, float mscale, const float* w_hh, const float* acts,
                       const float* call, float* dG, int T, int B, int H, void* workspace) {
    if (!w_hh || !acts || !call || !dG || !workspace || T <= 0 || !mtl_lstm_layer_supported(B, H)) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_counter(workspace, s)) return rc;
    LstmP p{nullptr, w_hh, nullptr, nullptr, const_cast<float*>(call), const_cast<float*>(acts), nullptr, mask, mscale, T, B, H,
            reinterpret_cast<unsigned*>(workspace), dx_up, dG};
    return dispatch_kc(H, [&](auto kc) { return launch_persistent<lstm_layer_bwd_kernel<kc()>>(H / LU, lstm_bwd_lds(B), 0, s, p); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// Sequence NLL of the LM's vocabulary projection (LM rescoring of finished beam hypotheses, utils/lm.py:42-155 of the reference):
// nll[r] = logsumexp_v(x_r . W_v + b_v) - (x_r . W_target + b_target) without ever writing the R x V logits.
//   stage 1 (lm_nll_partial_kernel): grid (row tiles of 64, vocabulary splits); a workgroup runs its rows against the 64-column blocks
//            of its split with exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain), keeps an online (max, sum-exp) per
//            row, picks up the target logit when its column passes, and writes (max, sum-exp, target logit) per (split, row);
//   stage 2 (lm_nll_merge_kernel): per row, the splits merged in split order -> row_nll;
//   stage 3 (lm_nll_seq_kernel): per sequence b, seq_nll[b] = sum over t of row_nll[t B + b] in t order.
// No atomics and fixed orders throughout: two runs give bit-identical results.
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NLL_RT = 64;            // rows per workgroup
constexpr int NLL_CT = 64;            // vocabulary columns per block
constexpr int NLL_KT = 32;            // k depth of one LDS stage
constexpr int NLL_TARGET_WGS = 512;   // stage-1 workgroups aimed for (two per CU; 1024 measured slower: 215 vs 168 us at H = 200)

struct NllSplit {
    int splits, blocks_per_split;
};
NllSplit nll_split(int R, int V) {
    const int nblk = (V + NLL_CT - 1) / NLL_CT, rt = (R + NLL_RT - 1) / NLL_RT;
    int s = (NLL_TARGET_WGS + rt - 1) / rt;
    s = s < 1 ? 1 : (s > nblk ? nblk : s);
    const int bps = (nblk + s - 1) / s;
    return NllSplit{(nblk + bps - 1) / bps, bps};      // every split holds at least one column
}

__device__ __forceinline__ void nll_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;                         // both empty
    s = s * expf(m - M) + s2 * expf(m2 - M);            // (an empty side has s == 0 and m == -inf: its term is 0)
    m = M;
}

__global__ __launch_bounds__(256) void lm_nll_partial_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W,
                                                            const float* __restrict__ bias, const long* __restrict__ target, int R,
                                                            int H, int V, int bps, float* __restrict__ part) {
    __shared__ float xs[NLL_KT][NLL_RT + 1];            // [k][row]
    __shared__ float wsm[NLL_KT][NLL_CT + 1];           // [k][column]
    __shared__ float lt[NLL_RT][NLL_CT + 1];            // the logits of one block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;            // this wave's 32 x 32 quarter of the 64 x 64 block
    const int r0 = blockIdx.x * NLL_RT;
    const int c_begin = blockIdx.y * bps * NLL_CT;
    const int c_end = min(V, c_begin + bps * NLL_CT);
    // epilogue ownership: thread (row er, strip q) scans the 16 columns [16 q, 16 q + 16) of every block
    const int er = tid >> 2, q = tid & 3;
    const int grow = r0 + er;
    const long tgt = grow < R ? target[grow] : -1;
    float m = -INFINITY, s = 0.f, tl = -INFINITY;
    for (int c0 = c_begin; c0 < c_end; c0 += NLL_CT) {
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the operands of a stage are fetched into registers while the matrix instructions of the stage before run (same values, same
        // order of the arithmetic: the results do not change)
        float px[NLL_RT * NLL_KT / 256], pw[NLL_RT * NLL_KT / 256];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int e = 0; e < NLL_RT * NLL_KT / 256; ++e) {
                const int idx = tid + 256 * e, kk = idx & (NLL_KT - 1), rr = idx / NLL_KT;
                const int k = k0 + kk, row = r0 + rr, col = c0 + rr;
                px[e] = (row < R && k < H) ? x[(long)row * ldx + k] : 0.f;
                pw[e] = (col < c_end && k < H) ? W[(long)col * H + k] : 0.f;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < H; k0 += NLL_KT) {
            __syncthreads();                              // the previous stage's operands (and the previous block's logits) are consumed
#pragma unroll
            for (int e = 0; e < NLL_RT * NLL_KT / 256; ++e) {
                const int idx = tid + 256 * e, kk = idx & (NLL_KT - 1), rr = idx / NLL_KT;
                xs[kk][rr] = px[e];
                wsm[kk][rr] = pw[e];
            }
            __syncthreads();
            if (k0 + NLL_KT < H) fetch(k0 + NLL_KT);
#pragma unroll
            for (int kk = 0; kk < NLL_KT; kk += 4) {
                float a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = xs[kk + (lane >> 4)][wr * 32 + i * 16 + (lane & 15)];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = wsm[kk + (lane >> 4)][wc * 32 + j * 16 + (lane & 15)];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        // C/D map of the 16x16 form: column lane & 15, row 4 (lane >> 4) + register
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) lt[wr * 32 + i * 16 + 4 * (lane >> 4) + g][wc * 32 + j * 16 + (lane & 15)] = acc[i][j][g];
        __syncthreads();
        float v[16], mb = -INFINITY;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int col = c0 + 16 * q + u;
            v[u] = col < c_end ? lt[er][16 * q + u] + (bias ? bias[col] : 0.f) : -INFINITY;
            mb = fmaxf(mb, v[u]);
            if (col == tgt) tl = v[u];
        }
        if (mb != -INFINITY) {
            const float M = fmaxf(m, mb);
            float sb = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) sb += expf(v[u] - M);      // (masked columns: exp(-inf) = 0)
            s = s * expf(m - M) + sb;
            m = M;
        }
    }
    // the four strips of a row sit in four adjacent lanes: butterfly merge (the same value in all four: both operations commute)
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64), t2 = __shfl_xor(tl, o, 64);
        nll_merge(m, s, m2, s2);
        tl = fmaxf(tl, t2);                               // at most one strip holds the target (-inf elsewhere)
    }
    if (q == 0 && grow < R) {
        float* p = part + ((long)blockIdx.y * R + grow) * 3;
        p[0] = m, p[1] = s, p[2] = tl;
    }
}

__global__ __launch_bounds__(256) void lm_nll_merge_kernel(const float* __restrict__ part, const long* __restrict__ target, int R, int V,
                                                          int splits, float* __restrict__ row_nll) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const long tgt = target[r];
    if (tgt < 0) {
        row_nll[r] = 0.f;                                 // skipped row (padding)
        return;
    }
    float m = -INFINITY, s = 0.f, tl = -INFINITY;
    for (int k = 0; k < splits; ++k) {
        const float* p = part + ((long)k * R + r) * 3;
        nll_merge(m, s, p[0], p[1]);
        tl = fmaxf(tl, p[2]);
    }
    row_nll[r] = (tgt < V && tl != -INFINITY) ? (m + logf(s)) - tl : __int_as_float(0x7fc00000);   // target out of range: NaN
}

__global__ __launch_bounds__(256) void lm_nll_seq_kernel(const float* __restrict__ row_nll, int T, int B, float* __restrict__ seq_nll) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += row_nll[(long)t * B + b];
    seq_nll[b] = acc;
}

// ---- LM evaluation: language-transition keys and keyed fp64 sums of the row NLLs -----------------------------------------------------
constexpr int KEYSUM_ROWS = 256;      // rows per workgroup of the partial pass (1024: 4 x the serial walk per owner thread, 0.14 ms at R = 8050)

__global__ __launch_bounds__(256) void lm_switch_keys_kernel(const long* __restrict__ ids, const long* __restrict__ target,
                                                            const unsigned char* __restrict__ lang, long eos_id, int R, int V,
                                                            int* __restrict__ key) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const long a = ids[r], b = target[r];
    int k = -1;
    if (a >= 0 && a < V && b >= 0 && b < V && a != eos_id && b != eos_id) k = (lang[a] ? 0 : 2) + (lang[b] ? 0 : 1);
    key[r] = k;
}

// One workgroup per KEYSUM_ROWS rows.  Thread t owns the keys k with k % 256 == t: it alone walks the chunk in row order and adds the rows
// of its keys (a run of equal keys in a register, flushed into the LDS slot of the key when the run ends), so no two threads ever touch
// one accumulator and the order of the additions is a function of the data alone.  part_sum / part_cnt: [workgroup][nkey].
__global__ __launch_bounds__(256) void nll_key_partial_kernel(const float* __restrict__ row_nll, const int* __restrict__ key, int seg_rows,
                                                             int R, int nkey, double* __restrict__ part_sum, int* __restrict__ part_cnt) {
    extern __shared__ double keysum_lds[];
    double* lsum = keysum_lds;                                                  // [nkey]
    float* sval = reinterpret_cast<float*>(lsum + nkey);                        // [KEYSUM_ROWS]
    int* skey = reinterpret_cast<int*>(sval + KEYSUM_ROWS);                     // [KEYSUM_ROWS]
    int* lcnt = skey + KEYSUM_ROWS;                                             // [nkey]
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * KEYSUM_ROWS;
    const int n = (int)min((long)KEYSUM_ROWS, (long)R - r0);
    for (int k = tid; k < nkey; k += 256) lsum[k] = 0.0, lcnt[k] = 0;
    for (int i = tid; i < n; i += 256) {
        const long r = r0 + i;
        const long k = key ? (long)key[r] : r / seg_rows;
        skey[i] = (k >= 0 && k < nkey) ? (int)k : -1;
        sval[i] = row_nll[r];
    }
    __syncthreads();
    if (tid < nkey) {
        int ck = -1, cc = 0;
        double cs = 0.0;
        for (int i = 0; i < n; ++i) {
            const int k = skey[i];
            if (k < 0 || (k & 255) != tid) continue;
            if (k != ck) {
                if (ck >= 0) lsum[ck] += cs, lcnt[ck] += cc;
                ck = k, cs = 0.0, cc = 0;
            }
            cs += (double)sval[i];
            ++cc;
        }
        if (ck >= 0) lsum[ck] += cs, lcnt[ck] += cc;
    }
    __syncthreads();
    double* ps = part_sum + (long)blockIdx.x * nkey;
    int* pc = part_cnt + (long)blockIdx.x * nkey;
    for (int k = tid; k < nkey; k += 256) ps[k] = lsum[k], pc[k] = lcnt[k];
}

__global__ __launch_bounds__(256) void nll_key_merge_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_cnt, int nblk,
                                                           int nkey, double* __restrict__ sum, int* __restrict__ count) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nkey) return;
    double s = 0.0;
    int c = 0;
    for (int b = 0; b < nblk; ++b) s += part_sum[(long)b * nkey + k], c += part_cnt[(long)b * nkey + k];     // workgroup order
    sum[k] = s;
    count[k] = c;
}

// The occurrence chains (mtl_embed_bwd's first / next) of EVERY bptt window of a batchified (S, B) stream in one launch: a workgroup
// per window, the window's ids in LDS, per row a scan back to the window's start (first) and forward to its end (next).  Exact and
// quadratic in the window's rows -- it runs once per stream, not once per step.
constexpr int CHAIN_MAX_ROWS = 4096;      // 32 KiB of ids in LDS

__global__ __launch_bounds__(256) void lm_window_chains_kernel(const long* __restrict__ ids, long S, int B, int bptt, int* __restrict__ first,
                                                              int* __restrict__ next) {
    extern __shared__ long wid[];
    const long i0 = (long)blockIdx.x * bptt;
    const long T = min((long)bptt, S - 1 - i0);
    const int R = (int)(T * B);               // <= CHAIN_MAX_ROWS (checked by the host)
    const long base = i0 * B;                 // base + R <= (S - 1) B: inside ids, first and next
    for (int r = threadIdx.x; r < R; r += 256) wid[r] = ids[base + r];
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += 256) {
        const long v = wid[r];
        int f = 1, nx = -1;
        for (int j = r - 1; j >= 0; --j)
            if (wid[j] == v) {
                f = 0;
                break;
            }
        for (int j = r + 1; j < R; ++j)
            if (wid[j] == v) {
                nx = j;
                break;
            }
        first[base + r] = f;
        next[base + r] = nx;
    }
}

}  // namespace

extern "C" {

int mtl_lm_window_chains_max_rows(void) { return CHAIN_MAX_ROWS; }

int mtl_lm_window_chains(void* stream, const long* ids, long S, int B, int bptt, int* first, int* next) {
    if (!ids || !first || !next || S < 2 || B < 1 || bptt < 1) return MTL_EINVAL;
    const long T = S - 1 < bptt ? S - 1 : (long)bptt;      // the longest window
    if (T * B > CHAIN_MAX_ROWS) return MTL_EINVAL;
    const long W = (S - 1 + bptt - 1) / bptt;
    if (W > 0x7fffffffL) return MTL_EINVAL;
    hipLaunchKernelGGL(lm_window_chains_kernel, dim3((unsigned)W), dim3(256), (size_t)(T * B) * sizeof(long), as_stream(stream), ids, S, B, bptt,
                       first, next);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_lm_switch_keys(void* stream, const long* ids, const long* target, const unsigned char* lang, long eos_id, int R, int V, int* key) {
    if (!ids || !target || !lang || !key || R < 1 || V < 1) return MTL_EINVAL;
    hipLaunchKernelGGL(lm_switch_keys_kernel, dim3((R + 255) / 256), dim3(256), 0, as_stream(stream), ids, target, lang, eos_id, R, V, key);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

long mtl_nll_key_sum_workspace(int R, int nkey) {
    if (R < 1 || nkey < 1 || nkey > MTL_NLL_MAX_KEYS) return MTL_EINVAL;
    return (long)((R + KEYSUM_ROWS - 1) / KEYSUM_ROWS) * nkey * 12;
}

int mtl_nll_key_sum(void* stream, const float* row_nll, const int* key, int seg_rows, int R, int nkey, double* sum, int* count, void* ws,
                    long ws_bytes) {
    if (!row_nll || !sum || !count || !ws || R < 1 || nkey < 1 || nkey > MTL_NLL_MAX_KEYS || (!key && seg_rows < 1)) return MTL_EINVAL;
    if (ws_bytes < mtl_nll_key_sum_workspace(R, nkey) || (reinterpret_cast<uintptr_t>(ws) & 7)) return MTL_EINVAL;
    const int nblk = (R + KEYSUM_ROWS - 1) / KEYSUM_ROWS;
    hipStream_t s = as_stream(stream);
    double* part_sum = static_cast<double*>(ws);
    int* part_cnt = reinterpret_cast<int*>(part_sum + (long)nblk * nkey);
    const size_t lds = (size_t)nkey * 12 + KEYSUM_ROWS * 8;                       // <= 50 KiB at MTL_NLL_MAX_KEYS
    hipLaunchKernelGGL(nll_key_partial_kernel, dim3(nblk), dim3(256), lds, s, row_nll, key, key ? 1 : seg_rows, R, nkey, part_sum, part_cnt);
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(nll_key_merge_kernel, dim3((nkey + 255) / 256), dim3(256), 0, s, part_sum, part_cnt, nblk, nkey, sum, count);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

long mtl_lm_nll_workspace(int R, int V) {
    if (R <= 0 || V <= 0) return 0;
    return (long)nll_split(R, V).splits * R * 3 * 4;
}

int mtl_lm_nll_fwd(void* stream, const float* x, int ldx, const float* W, const float* bias, const long* target, int R, int H, int V,
                   int B, float* row_nll, float* seq_nll, void* ws, long ws_bytes) {
    if (!x || !W || !target || !row_nll || !ws || R <= 0 || H <= 0 || V <= 0 || B <= 0 || R % B != 0 || ldx < H) return MTL_EINVAL;
    if (ws_bytes < mtl_lm_nll_workspace(R, V) || (reinterpret_cast<uintptr_t>(ws) & 3)) return MTL_EINVAL;
    const NllSplit sp = nll_split(R, V);
    hipStream_t s = as_stream(stream);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(lm_nll_partial_kernel, dim3((R + NLL_RT - 1) / NLL_RT, sp.splits), dim3(256), 0, s, x, ldx, W, bias, target, R, H,
                       V, sp.blocks_per_split, part);
    MTL_CHECK_LAUNCH();
    hipLaunchKernelGGL(lm_nll_merge_kernel, dim3((R + 255) / 256), dim3(256), 0, s, part, target, R, V, sp.splits, row_nll);
    MTL_CHECK_LAUNCH();
    if (seq_nll) {
        hipLaunchKernelGGL(lm_nll_seq_kernel, dim3((B + 255) / 256), dim3(256), 0, s, row_nll, R / B, B, seq_nll);
        MTL_CHECK_LAUNCH();
    }
    return MTL_OK;
}

}  // extern "C"
