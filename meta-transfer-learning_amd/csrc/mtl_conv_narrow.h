// The 32-channel 3 x 3 shapes of the large_cnn front-end (Conv 32 -> 32 + pool, Conv 32 -> 64) on the exact bf16 split ("x3"):
// what mtl_mfma.hip's x3 entry points hand to mtl_conv_narrow.hip.  Host-side interface only; the kernels are in the .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

enum { NARROW_RELU = 0, NARROW_POOL = 1, NARROW_DGRAD = 2 };

// One convolution-shaped launch: K reduction channels -> N output channels (a data gradient: K = the forward's Cout, N = its Cin, on
// the tap-reversed image w3d of conv_wprep_x3_kernel).  Pointers and task strides as in ConvX3P (mtl_mfma.hip).
struct NarrowConvP {
    const float* x;            // source (B, T, F, K), or the pooled gradient (B, Tp, Fp, K) when am_in is given
    const uint8_t* am_in;      // arg-max codes of the pooled source (un-pooling), else nullptr
    const unsigned char* w3;   // [3 pieces][K-tile = tap * K / 32 + k / 32][N rows][32 bf16, x3_swz]
    const float* bias;         // forwards
    const float* act;          // data gradients: the forward activation (B, T, F, N) whose sign gates the output
    float* y;                  // (B, T, F, N), pooled forward: (B, Tp, Fp, N)
    uint8_t* am_out;           // pooled forward: arg-max codes, one byte per pooled element
    int B, T, F, K, N, Tp, Fp; // B counts the samples of ALL tasks
    int Te, Fe;                // extent the pixel tiles cover (pooled forward: 2 Tp x 2 Fp)
    int Bt;                    // samples per task
    long sW, sBias;            // task k: weights at w3 + k sW bytes, bias at bias + k sBias floats
    const int* widths;         // optional frame counts per task: tile rows beyond ceil((widths[k] >> wshift) / 8) are skipped
    int wshift;
    int ntf, ntt;              // (set by the launcher)
};

bool narrow_conv_serves(int K, int N, bool unpool, int epi);
int narrow_conv_launch(hipStream_t s, NarrowConvP p, bool unpool, int epi);

// Weight gradient dW[tap][ci][co] = sum over pixels x[pixel + tap][ci] dy[pixel][co] for Cin = 32, Cout = 32 | 64; the bias gradient
// (column sums of dy) rides along.  The launch writes `slots` partial slabs [9 Cin][Cout] (+ [Cout] bias sums) into the workspace,
// dealt to the tasks in equal contiguous ranges; wgrad_reduce_kernel (mtl_mfma.hip) sums slots / tasks of them per task.
struct NarrowWgradP {
    const float* x;            // (tasks B, T, F, 32)
    const float* dy;           // (tasks B, T, F, Cout) or pooled (tasks B, Tp, Fp, Cout) with am
    const uint8_t* am;
    float* partial;            // [slots][9 * 32][Cout]
    float* bias_part;          // [slots][Cout] or nullptr
    int B, T, F, Ty, Fy, Tp, Fp, Cout;   // B: samples of ONE task; Ty x Fy: extent over which dy can be non-zero
    int tasks;
    int ntf, ntt, tiles;       // (set by the launcher) pixel tiles of one task
};

bool narrow_wgrad_serves(int Cin, int Cout);
int narrow_wgrad_slots(void);
int narrow_wgrad_launch(hipStream_t s, NarrowWgradP p);
