// GRU kernels for gfx950 (MI355X): the cell of one time step (element-wise) and the persistent layer -- all T time steps of one layer
// in ONE launch per direction (lm/model/rnn_model.py:21 nn.GRU over a bptt window, `--model GRU`).
//
// The cell arithmetic (gru_cell_act / gru_cell_grad, torch gate order r | z | n, q = gh_n saved as the fourth activation) is in
// mtl_rnn_cell.h.  The kernels write two gate-gradient tensors:
//   dgx = [da_r, da_z, da_n] (-> W_ih, b_ih, the input gradient)   dgh = [da_r, da_z, dq] (-> W_hh, b_hh, dh_rec(t - 1) = dgh W_hh)
//
// The persistent kernels keep the ownership, the hand-off and the workspace of the LSTM's (mtl_lstm.hip): workgroup w owns the hidden
// units [8 w, 8 w + 8) for the whole sequence, its 24 rows of W_hh (rows g H + j) stay in registers, one grid-wide hand-off per
// step, fixed-order reductions (bitwise reproducible), every spin bounded.  Shared with the LSTM through mtl_handoff.h: the hand-off,
// the backward's row-split partial product, the width dispatch, the launch and the counter reset.
#include "mtl_handoff.h"
#include "mtl_rnn_cell.h"

namespace {

struct GruP {
    const float *gx, *whh, *bhh;
    float *hall, *acts, *xout;
    const uint8_t* mask;
    float mscale;
    int T, B, H;
    unsigned* sync;                           // [0] arrivals (zeroed by the launcher), [1] error word
    // backward
    const float* dx_up;
    float *dgx, *dgh;
};

// ------------------------------------------------------------------------------------------------------ one time step, element-wise
__global__ __launch_bounds__(256) void gru_cell_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ gh,
                                                           const float* __restrict__ h_prev, float* __restrict__ acts,
                                                           float* __restrict__ h, float* __restrict__ h_drop,
                                                           const uint8_t* __restrict__ mask, float mscale, int B, int H) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * H) return;
    const int b = e / H, j = e - b * H;
    const long g3 = (long)b * 3 * H + j, a4 = (long)b * 4 * H + j;
    const GruAct a = gru_cell_act(gx, gh, g3, H, h_prev + e);
    acts[a4] = a.r;
    acts[a4 + H] = a.z;
    acts[a4 + 2 * H] = a.n;
    acts[a4 + 3 * H] = a.q;
    h[e] = a.h;
    if (h_drop) h_drop[e] = dropped(a.h, mask, e, mscale);
}

__global__ __launch_bounds__(256) void gru_cell_bwd_kernel(const float* __restrict__ dh_up, const uint8_t* __restrict__ mask,
                                                           float mscale, const float* __restrict__ dh_rec, const float* carry_in,
                                                           const float* __restrict__ acts, const float* __restrict__ h_prev,
                                                           float* __restrict__ dgx, float* __restrict__ dgh, float* carry_out, int B,
                                                           int H) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * H) return;
    const int b = e / H, j = e - b * H;
    const long g3 = (long)b * 3 * H + j, a4 = (long)b * 4 * H + j;
    float dh = dh_up ? dropped(dh_up, mask, e, mscale) : 0.f;
    if (dh_rec) dh += dh_rec[e];
    if (carry_in) dh += carry_in[e];
    const GruGrad g = gru_cell_grad(dh, acts[a4], acts[a4 + H], acts[a4 + 2 * H], acts[a4 + 3 * H], h_prev[e]);
    dgx[g3] = g.da_r, dgx[g3 + H] = g.da_z, dgx[g3 + 2 * H] = g.da_n;
    dgh[g3] = g.da_r, dgh[g3 + H] = g.da_z, dgh[g3 + 2 * H] = g.dq;
    carry_out[e] = g.carry;
}

// ------------------------------------------------------------------------------------------------------------- persistent forward
// floats between the chunk planes of the partial-sum buffer [chunk][B][24 rows]: = 8 mod 64, so the 8 chunks x 8 units of a wave
// write 64 different LDS banks
__host__ __device__ constexpr int red_stride(int B) {
    const int rs = B * 24;
    return rs + (72 - rs % 64) % 64;
}
// the staged state is kept as [B][16 chunks][KH + 4]: one float4 of padding per chunk, so the 8 chunks a wave reads together (16-byte
// reads KH floats apart: the same banks for KH = 16 / 32) fall into different banks
template <int KC>
constexpr int state_stride() { return 8 * KC + 4 * NCH; }
// dynamic LDS of gru_layer_fwd_kernel: the staged state [B][state_stride] + the chunk partials [NCH][red_stride]
template <int KC>
constexpr int gru_fwd_lds(int B) { return (B * state_stride<KC>() + NCH * red_stride(B)) * 4; }

// B x H floats written by other workgroups -> LDS in the padded layout, 256 threads.  16-byte `sc1` loads, eight in flight behind ONE
// wait inside the same statement (early-clobber outputs: the compiler cannot touch the destinations before the data has landed);
// lanes past the end re-read the last 16 bytes instead of branching around the statement.
template <int KC>
__device__ __forceinline__ void stage_state(float* lds, const float* src, int n4, int tid) {
    constexpr int H4 = 2 * KC, KH4 = KC / 8, HP4 = state_stride<KC>() / 4;
#pragma unroll 1
    for (int base = 0; base < n4; base += 8 * 256) {
        float4 v[8];
        const float* a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + tid + 256 * k;
            a[k] = src + 4 * (long)(idx < n4 ? idx : n4 - 1);
        }
        asm volatile(
            "global_load_dwordx4 %0, %8, off sc1\n\t"
            "global_load_dwordx4 %1, %9, off sc1\n\t"
            "global_load_dwordx4 %2, %10, off sc1\n\t"
            "global_load_dwordx4 %3, %11, off sc1\n\t"
            "global_load_dwordx4 %4, %12, off sc1\n\t"
            "global_load_dwordx4 %5, %13, off sc1\n\t"
            "global_load_dwordx4 %6, %14, off sc1\n\t"
            "global_load_dwordx4 %7, %15, off sc1\n\t"
            "s_waitcnt vmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
            : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7])
            : "memory");
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + tid + 256 * k;
            if (idx < n4) {
                const int b = idx / H4, c4 = idx - b * H4;
                reinterpret_cast<float4*>(lds)[b * HP4 + c4 + c4 / KH4] = v[k];
            }
        }
    }
}

// Thread (unit = tid & 7, chunk = (tid >> 3) & 15, half = tid >> 7) holds the THREE gate rows of its unit over the chunk's H / 16 columns
// (<= 96 registers) and multiplies them with the batch rows b = half, half + 2, ...: every LDS read of the state feeds three rows and
// a thread walks half the batch (the product is LDS-bound: 3/4 of the LSTM kernel's rows at less than half its LDS reads).  The 16
// chunk partials of an output are summed in a fixed order by the thread (b, unit) that applies the cell and keeps h in a register.
template <int KC>      // H = 8 KC
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void gru_layer_fwd_kernel(GruP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int H = 8 * KC, KH = KC / 2, HP = state_stride<KC>();
    const int B = p.B, T = p.T, RS = red_stride(B);
    float* hs = sm;                     // [B][HP]
    float* red = sm + B * HP;           // [16 chunks][RS >= B x 24 rows]
    const int tid = threadIdx.x, cu = tid & 7, kc = (tid >> 3) & (NCH - 1), half = tid >> 7;
    const int j0 = blockIdx.x * LU, cj = j0 + cu;
    const unsigned nwg = gridDim.x;
    float w[3][KH];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const float* wrow = p.whh + (long)(g * H + cj) * H + kc * KH;
#pragma unroll
        for (int i = 0; i < KH; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(wrow + i);
            w[g][i] = v.x, w[g][i + 1] = v.y, w[g][i + 2] = v.z, w[g][i + 3] = v.w;
        }
    }
    const bool cell = tid < B * LU;
    const int cb = tid / LU;            // (tid % LU == cu)
    float bias[3] = {0.f, 0.f, 0.f};
    float h_prev = 0.f;
    if (cell) {
#pragma unroll
        for (int g = 0; g < 3; ++g) bias[g] = p.bhh[g * H + cj];
        h_prev = p.hall[(long)cb * H + cj];
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float gxv[3] = {0.f, 0.f, 0.f};                         // this step's input contributions: requested before the wait
        if (cell) {
#pragma unroll
            for (int g = 0; g < 3; ++g) gxv[g] = p.gx[((long)t * B + cb) * 3 * H + g * H + cj];
        }
        if (t > 0) grid_wait(p.sync, (unsigned)t * nwg);        // every workgroup has published h_t
        stage_state<KC>(hs, p.hall + (long)t * B * H, B * H / 4, tid);
        __syncthreads();
#pragma unroll 1
        for (int b = half; b < B; b += 2) {
            const float* hb = hs + b * HP + kc * (KH + 4);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int i = 0; i < KH; i += 4) {
                const float4 hv = *reinterpret_cast<const float4*>(hb + i);
                a0 = fmaf(w[0][i], hv.x, a0), a1 = fmaf(w[1][i], hv.x, a1), a2 = fmaf(w[2][i], hv.x, a2);
                a0 = fmaf(w[0][i + 1], hv.y, a0), a1 = fmaf(w[1][i + 1], hv.y, a1), a2 = fmaf(w[2][i + 1], hv.y, a2);
                a0 = fmaf(w[0][i + 2], hv.z, a0), a1 = fmaf(w[1][i + 2], hv.z, a1), a2 = fmaf(w[2][i + 2], hv.z, a2);
                a0 = fmaf(w[0][i + 3], hv.w, a0), a1 = fmaf(w[1][i + 3], hv.w, a1), a2 = fmaf(w[2][i + 3], hv.w, a2);
            }
            float* o = red + kc * RS + b * 24 + cu;
            o[0] = a0, o[8] = a1, o[16] = a2;
        }
        __syncthreads();
        if (cell) {
            const long row = (long)t * B + cb;
            float gh[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) s += red[c * RS + cb * 24 + g * 8 + cu];
                gh[g] = s + bias[g];
            }
            const GruAct a = gru_cell_act(gxv, gh, 0, 1, &h_prev);
            float* ac = p.acts + row * 4 * H + cj;
            ac[0] = a.r, ac[H] = a.z, ac[2 * H] = a.n, ac[3 * H] = a.q;
            const long e = row * H + cj;
            store_shared(p.hall + e + (long)B * H, a.h);       // hall[t + 1]: read by every workgroup in the next step
            if (p.xout) p.xout[e] = dropped(a.h, p.mask, e, p.mscale);
            h_prev = a.h;
        }
        if (t + 1 < T) grid_arrive(p.sync);      // (its barrier also orders this step's LDS reads before the next step's writes)
    }
}

// ------------------------------------------------------------------------------------------------------------ persistent backward
// Same ownership in reverse time, as lstm_layer_bwd_kernel: the recurrent gradient dh_rec_t = dgh_{t+1} . W_hh is split by ROWS --
// workgroup w multiplies the 24 columns of dgh_{t+1} it has just produced (in LDS) with its 24 rows of W_hh for all H outputs
// (rowsplit_partial, mtl_handoff.h) and publishes that partial (B x H, write-through); after the hand-off every workgroup sums the
// partials of its own 8 units over the workgroups in a fixed order.  Two partial buffers alternate with the
// step parity.  The direct carry dh' z stays in the owning thread's register: no hand-off.
//
// The sum over the N = H / 8 partials of one (batch row, unit): N `sc1` dword loads (uniform base of partial k in SGPRs + this lane's
// byte offset) ALL in flight behind one wait.  As relaxed agent-scope atomic loads the compiler keeps them in program order with a
// wait after every pair: 32 memory round trips per step at H = 512.  Every destination is named by the statements after the loads,
// so none is read, copied or reused before the wait; the summation order (even partials, odd partials, then the two sums) is fixed.
template <int N>
__device__ __forceinline__ float gather_partials(const float* base, long stride, unsigned lane_bytes) {
    static_assert(N % 16 == 0, "partials are named in groups of 16");
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
        asm volatile("global_load_dword %0, %1, %2 sc1" : "=v"(v[k]) : "v"(lane_bytes), "s"(base + k * stride) : "memory");
#pragma unroll
    for (int k = 0; k < N; k += 16) {
        if (k == 0)
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]),
                           "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])
                         :
                         : "memory");
        else
            asm volatile(""
                         : "+v"(v[k]), "+v"(v[k + 1]), "+v"(v[k + 2]), "+v"(v[k + 3]), "+v"(v[k + 4]), "+v"(v[k + 5]), "+v"(v[k + 6]),
                           "+v"(v[k + 7]), "+v"(v[k + 8]), "+v"(v[k + 9]), "+v"(v[k + 10]), "+v"(v[k + 11]), "+v"(v[k + 12]),
                           "+v"(v[k + 13]), "+v"(v[k + 14]), "+v"(v[k + 15])
                         :
                         : "memory");
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < N; k += 2) s0 += v[k], s1 += v[k + 1];
    return s0 + s1;
}

template <int KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void gru_layer_bwd_kernel(GruP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int H = 8 * KC;
    constexpr int JT = KC > 32 ? 2 : 1;           // output units per thread in the partial product
    const int B = p.B, T = p.T;
    float* dgs = sm;                              // [B][24]: this workgroup's columns of dgh_t (local row = gate * 8 + unit)
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * LU;
    const unsigned nwg = gridDim.x;
    const int jt = tid * JT;                      // first output unit of this thread
    const bool active = jt < H;
    float w[24][JT];
    if (active) load_rowsplit_weights<8 * KC>(w, p.whh, jt);
    float* P = reinterpret_cast<float*>(p.sync) + HDR;        // two buffers of [nwg][B][H] behind the header
    const long pbuf = (long)nwg * B * H;
    const bool cell = tid < B * LU;
    const int cb = tid / LU, cu = tid % LU, cj = j0 + cu;
    float carry = 0.f;
#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
        float dh_rec = 0.f;
        // this step's own operands do not depend on the other workgroups: requested before the wait
        float dh_up = 0.f, ar = 0.f, az = 0.f, an = 0.f, aq = 0.f, hprev = 0.f;
        if (cell) {
            const long row = (long)t * B + cb;
            const long e = row * H + cj;
            dh_up = p.dx_up ? dropped(p.dx_up, p.mask, e, p.mscale) : 0.f;
            const float* ac = p.acts + row * 4 * H + cj;
            ar = ac[0], az = ac[H], an = ac[2 * H], aq = ac[3 * H];
            hprev = p.hall[e];                                  // hall[t]: written by the forward launch
        }
        if (t < T - 1) {
            grid_wait(p.sync, (unsigned)(T - 1 - t) * nwg);     // every workgroup has published its partial of step t + 1
            // (nwg == KC: one partial per workgroup)
            if (cell) dh_rec = gather_partials<KC>(P + ((t + 1) & 1) * pbuf, (long)B * H, (unsigned)(cb * H + cj) * 4u);
        }
        if (cell) {
            const long row = (long)t * B + cb;
            float dh = dh_up;
            if (t < T - 1) dh = (dh + dh_rec) + carry;          // (the per-step path's order of the three terms)
            const GruGrad g = gru_cell_grad(dh, ar, az, an, aq, hprev);
            float* gx = p.dgx + row * 3 * H + cj;
            gx[0] = g.da_r, gx[H] = g.da_z, gx[2 * H] = g.da_n;
            float* gh = p.dgh + row * 3 * H + cj;
            gh[0] = g.da_r, gh[H] = g.da_z, gh[2 * H] = g.dq;
            float* l = dgs + cb * 24 + cu;
            l[0] = g.da_r, l[8] = g.da_z, l[16] = g.dq;
            carry = g.carry;
        }
        if (t > 0) {
            __syncthreads();
            if (active) rowsplit_partial(w, dgs, P + (t & 1) * pbuf + (long)blockIdx.x * B * H + jt, B, H);
            grid_arrive(p.sync);      // (its barrier also orders the reads of dgs before the next step's writes)
        }
    }
}

}  // namespace

extern "C" {

int mtl_gru_cell_fwd(void* stream, const float* gx, const float* gh, const float* h_prev, float* acts, float* h, float* h_drop,
                     const unsigned char* mask, float mscale, int B, int H) {
    if (!gx || !gh || !h_prev || !acts || !h || B <= 0 || H <= 0 || (long)B * H > 0x7fffffffL / 4) return MTL_EINVAL;
    hipLaunchKernelGGL(gru_cell_fwd_kernel, dim3((B * H + 255) / 256), dim3(256), 0, as_stream(stream), gx, gh, h_prev, acts, h, h_drop,
                       mask, mscale, B, H);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_gru_cell_bwd(void* stream, const float* dh_up, const unsigned char* mask, float mscale, const float* dh_rec,
                     const float* carry_in, const float* acts, const float* h_prev, float* dgx, float* dgh, float* carry_out, int B,
                     int H) {
    if (!acts || !h_prev || !dgx || !dgh || !carry_out || B <= 0 || H <= 0 || (long)B * H > 0x7fffffffL / 4) return MTL_EINVAL;
    hipLaunchKernelGGL(gru_cell_bwd_kernel, dim3((B * H + 255) / 256), dim3(256), 0, as_stream(stream), dh_up, mask, mscale, dh_rec,
                       carry_in, acts, h_prev, dgx, dgh, carry_out, B, H);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_gru_layer_supported(int B, int H) { return mtl_lstm_layer_supported(B, H); }

int mtl_gru_layer_fwd(void* stream, const float* gx, const float* w_hh, const float* b_hh, float* hall, float* acts, float* xout,
                      const unsigned char* mask, float mscale, int T, int B, int H, void* workspace) {
    if (!gx || !w_hh || !b_hh || !hall || !acts || !workspace || T <= 0 || !mtl_gru_layer_supported(B, H)) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_counter(workspace, s)) return rc;
    GruP p{gx, w_hh, b_hh, hall, acts, xout, mask, mscale, T, B, H, reinterpret_cast<unsigned*>(workspace), nullptr, nullptr, nullptr};
    return dispatch_kc(H, [&](auto kc) {
        return launch_persistent<gru_layer_fwd_kernel<kc()>>(H / LU, gru_fwd_lds<kc()>(B), gru_fwd_lds<kc()>(MAXB), s, p);
    });
}

int mtl_gru_layer_bwd(void* stream, const float* dx_up, const unsigned char* mask, float mscale, const float* w_hh, const float* acts,
                      const float* hall, float* dgx, float* dgh, int T, int B, int H, void* workspace) {
    if (!w_hh || !acts || !hall || !dgx || !dgh || !workspace || T <= 0 || !mtl_gru_layer_supported(B, H)) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    if (const int rc = reset_counter(workspace, s)) return rc;
    GruP p{nullptr, w_hh, nullptr, const_cast<float*>(hall), const_cast<float*>(acts), nullptr, mask, mscale, T, B, H,
           reinterpret_cast<unsigned*>(workspace), dx_up, dgx, dgh};
    return dispatch_kc(H, [&](auto kc) { return launch_persistent<gru_layer_bwd_kernel<kc()>>(H / LU, B * 24 * 4, 0, s, p); });
}

}  // extern "C"
