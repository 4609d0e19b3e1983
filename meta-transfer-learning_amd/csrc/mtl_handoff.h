// What the persistent recurrent-layer kernels (mtl_lstm.hip, mtl_gru.hip) share besides the cell arithmetic (mtl_rnn_cell.h):
//   * the layout of their workspace and the grid-wide hand-off (grid_wait / grid_arrive / store_shared);
//   * the row-split partial product of the layer kernels' backward (load_rowsplit_weights / rowsplit_partial);
//   * the host side of a launch: width dispatch (dispatch_kc), the launch itself with its dynamic-LDS limit (launch_persistent) and
//     the re-zeroing of the workspace header (reset_counter / reset_flags).
#pragma once
#include <type_traits>

#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

constexpr int LU = 8;                        // hidden units per workgroup
constexpr int NCH = 16;                      // k chunks of the forward's recurrent product
constexpr int MAXB = 32;                     // largest batch of a persistent launch (mtl_lstm_layer_supported)
constexpr unsigned SPIN_LIMIT = 1u << 22;    // polls before a wait gives up (~seconds): sets the error word
constexpr int HDR = 1024;                    // workspace header in 4-byte words: [0] arrival counter (single-layer kernels), [1] error word,
                                             // [64 + 64 g ..): the per-workgroup step flags of group g of the stack kernels
constexpr int MAXL = MTL_LSTM_MAX_LAYERS;
constexpr long PBUF = 64L * 32 * 512;        // largest [nwg][B][H] partial buffer, floats

// Hand-off without cache maintenance (guide, Guideline 16 form R1): the payload that crosses workgroups (h_t, dG_t) is stored
// write-through (relaxed agent-scope atomic stores = `global_store ... sc1`) and read with `sc1` loads (relaxed agent-scope atomic
// loads: served below the reader's L1), so neither an L2 write-back (release fence, 2-6 us with fresh dirty lines) nor an L1
// invalidate (acquire fence, 1.7 us) is paid per step; the flag follows the payload behind `s_waitcnt vmcnt(0)`.
__device__ __forceinline__ void grid_wait(unsigned* sync, unsigned target) {
    if (threadIdx.x == 0) {
        unsigned spins = 0;
        while (__hip_atomic_load(&sync[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (++spins > SPIN_LIMIT) {
                __hip_atomic_store(&sync[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void grid_arrive(unsigned* sync) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through stores are acknowledged
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&sync[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_shared(float* q, float v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Backward, recurrent gradient split by ROWS: a workgroup multiplies the NR columns of the gate gradient it has just produced (dgs,
// LDS [B][NR], local row = gate * 8 + unit) with its NR rows of W_hh (rows gate H + j0 + unit) for all H outputs.  Thread: the JT
// output units from jt on, NR x JT weights in registers, the gradient operand an LDS broadcast, ONE fmaf chain per output in row
// order; the partial goes out write-through (two units as one 64-bit store).
// (The compiler simplifies a helper on its own before inlining it, so the weight load takes the width as a template parameter and
// derives the workgroup's first unit itself: with what the kernels know -- H a constant, j0 a multiple of 8 -- it forms the row
// addresses the way the written-out loops did.)
template <int H, int NR, int JT>
__device__ __forceinline__ void load_rowsplit_weights(float (&w)[NR][JT], const float* whh, int jt) {
    const int j0 = blockIdx.x * LU;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float* q = whh + (long)((r >> 3) * H + j0 + (r & 7)) * H + jt;
#pragma unroll
        for (int c = 0; c < JT; ++c) w[r][c] = q[c];
    }
}
template <int NR, int JT>
__device__ __forceinline__ void rowsplit_partial(const float (&w)[NR][JT], const float* dgs, float* out, int B, int H) {
#pragma unroll 1
    for (int b = 0; b < B; ++b) {
        const float* gb = dgs + b * NR;
        float a[JT];
#pragma unroll
        for (int c = 0; c < JT; ++c) a[c] = 0.f;
#pragma unroll
        for (int r = 0; r < NR; r += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(gb + r);
#pragma unroll
            for (int c = 0; c < JT; ++c) {
                a[c] = fmaf(gv.x, w[r][c], a[c]);
                a[c] = fmaf(gv.y, w[r + 1][c], a[c]);
                a[c] = fmaf(gv.z, w[r + 2][c], a[c]);
                a[c] = fmaf(gv.w, w[r + 3][c], a[c]);
            }
        }
        if (JT == 2) {
            const unsigned long long u = (unsigned long long)__builtin_bit_cast(unsigned, a[0]) |
                                         ((unsigned long long)__builtin_bit_cast(unsigned, a[JT - 1]) << 32);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(out + (long)b * H), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            store_shared(out + (long)b * H, a[0]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- host
// f(std::integral_constant<int, KC>) for the supported widths H = 8 KC (the callers have checked mtl_lstm_layer_supported)
template <class F>
int dispatch_kc(int H, F&& f) {
    switch (H / LU) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 48: return f(std::integral_constant<int, 48>{});
        default: return f(std::integral_constant<int, 64>{});
    }
}

// One persistent launch: `grid` workgroups of 256 threads with `lds` bytes of dynamic LDS.  lds_max != 0: the kernel's layout can
// exceed the default limit, which is raised to lds_max (the layout's size at B = MAXB) once per kernel instantiation.
template <auto Kernel, class P>
int launch_persistent(int grid, int lds, int lds_max, hipStream_t s, const P& p) {
    static const int attr = (!lds_max || hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                             lds_max) == hipSuccess) ? MTL_OK : MTL_ELAUNCH;
    if (attr) return attr;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(256), lds, s, p);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

// Before every launch, on its stream.  The error word [1] is sticky: nothing here clears it.
inline int reset_counter(void* workspace, hipStream_t s) {      // the arrival counter of the single-layer kernels
    return hipMemsetAsync(workspace, 0, 4, s) == hipSuccess ? MTL_OK : MTL_ELAUNCH;
}
inline int reset_flags(void* workspace, hipStream_t s) {        // the step flags of the stack kernels
    return hipMemsetAsync(static_cast<char*>(workspace) + 256, 0, (HDR - 64) * 4, s) == hipSuccess ? MTL_OK : MTL_ELAUNCH;
}

}  // namespace
