// Grid-wide hand-off of the persistent recurrent-layer kernels (mtl_lstm.hip, mtl_gru.hip) and the layout of their shared workspace.
#pragma once
#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

constexpr int LU = 8;                        // hidden units per workgroup
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

}  // namespace
