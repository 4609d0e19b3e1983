/* mtl_hip.h -- C ABI of libmtl_hip.so: the MI355X (gfx950) kernels of the meta-transfer-learning hot path.
 *
 * Drop-in boundary.  The reference (audioku/meta-transfer-learning) has no FFI layer: its
 * hot path is Python calling stock PyTorch ops.  This library supplies, as hand-written HIP, every op that
 * path issues; each entry point cites the reference call site(s) it replaces (paths relative to the reference
 * repository root).  The Python host layer (meta-transfer-learning_amd/) binds these with ctypes and keeps the
 * reference's own Python signatures (Transformer.forward, TransientTrainer.train, ...).  INTEGRATION.md shows
 * the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless named `*_host`; the library never
 *     allocates, frees or retains memory.  Scratch space is passed in (`workspace`, size from *_workspace()).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No call synchronises the device.
 *   - return 0 on success, a negative errno-style code otherwise (-22 bad argument, -5 launch failure);
 *     nothing throws or aborts.  Re-entrant; one host thread per device.
 *   - all tensors fp32 row-major unless stated; token ids int64 (`long`), lengths int32.
 *   - activations inside the conv stack are channels-last with TIME outermost: (B, T, F, C).
 *   - "accum" outputs are ADDED to (gradient accumulation semantics of .backward()).
 *   - all reductions are fixed-order (no floating-point atomics): results are run-to-run deterministic.
 */
#ifndef MTL_HIP_H
#define MTL_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

int mtl_abi_version(void);

/* ---- GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) -------------------------------------------
 * C[z] = epilogue( alpha * opA(A[z]) . opB(B[z]) ),  z = 0..batch-1,  operand z at  base + (z/H)*s?b + (z%H)*s?h
 *   transA = 0: A is M x K (lda)   | 1: A is stored K x M (lda)
 *   transB = 0: B is K x N (ldb)   | 1: B is stored N x K (ldb)
 *   epilogue: + bias[n] (nullable) ; ReLU if flags&MTL_GEMM_RELU ; zero where gate[m*ldg+n] <= 0 (nullable,
 *             same batch offsets as C) ; += C if flags&MTL_GEMM_ACCUM.
 *   sBias: bias stride (floats) of the outer batch index b (0 = one bias vector for every item) -- lets the three Q/K/V
 *             projections of an attention block, whose parameters sit at a constant stride in the flat buffer, run as ONE call.
 *   workspace (nullable): when the output has too few tiles (x batch items) to fill the 256 CUs, K is split over the grid
 *             into workspace slabs that a second kernel sums in fixed order (deterministic split-K).
 * Replaces nn.Linear forward/backward (modules/encoder.py:72; modules/common_layers.py:130,287-289,303;
 * modules/decoder.py:108-110) and torch.bmm (modules/common_layers.py:321,329) incl. the permute/contiguous
 * copies at common_layers.py:291-293,301 (heads are addressed by stride instead). */
#define MTL_GEMM_RELU 1
#define MTL_GEMM_ACCUM 2
int mtl_gemm_f32(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                 const float* B, int ldb, float* C, int ldc, const float* bias, const float* gate, int ldg, int flags,
                 int batch, int H, long sAb, long sAh, long sBb, long sBh, long sCb, long sCh, long sBias, float* workspace,
                 long workspace_bytes);

/* mtl_gemm_f32 with two extensions, and a small-tile engine (32 x 32 tiles on v_mfma_f32_16x16x4_f32, no workspace, no second
 * launch) for products whose 64 x 64 tiling would leave most of the 256 CUs idle (< 192 tiles):
 *   kbatch > 1: C = epilogue( alpha * sum_{z<kbatch} opA(A + z*sAk) . opB(B + z*sBk) ) -- the K loop runs over the z items inside
 *               ONE launch (dx of the Q/K/V low-rank a-stages: three serialised accumulate launches before);
 *   rowsum (nullable, transA only): rowsum[(z/H)*sRowsum + m] += sum_k opA(A)[m][k] -- the bias gradient colsum(dy) of
 *               dW = dy^T . x as a by-product of the weight-gradient product (fixed-order reduction).
 * Products that fill the chip (and the few-tile very-long-K ones) are forwarded to mtl_gemm_f32 unchanged. */
int mtl_gemm_f32_ex(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                    const float* B, int ldb, float* C, int ldc, const float* bias, const float* gate, int ldg, int flags,
                    int batch, int H, long sAb, long sAh, long sBb, long sBh, long sCb, long sCh, long sBias, int kbatch, long sAk,
                    long sBk, float* rowsum, long sRowsum, float* workspace, long workspace_bytes,
                    long sBiasH, long sRowsumH /* bias / rowsum strides of the INNER batch index (z % H); sBias / sRowsum belong to z / H:
                                                  e.g. the K and V projections (inner) of all decoder layers (outer) in one launch */);
/* mtl_gemm_f32_ex with a THIRD, outermost batch level -- the tasks of a meta-step (trainer/asr/transient_trainer.py:178-237: every
 * task's passes are independent given theta0) batched into one launch: batch = tasks * (items per task); item z belongs to task
 * zt = z / (batch / tasks) and its operands sit at base + zt * s?t + (the two-level offsets of z % (batch / tasks)).  The weights
 * of the validation passes differ per task (theta'_t = theta0 - alpha g_t, a stack with stride sBt; 0 for the shared theta0 of
 * the training passes), per-task gradients accumulate into a stack (sCt / sRowsumT). */
int mtl_gemm_f32_tb(void* stream, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                    const float* B, int ldb, float* C, int ldc, const float* bias, const float* gate, int ldg, int flags,
                    int batch, int H, long sAb, long sAh, long sBb, long sBh, long sCb, long sCh, long sBias, int kbatch, long sAk,
                    long sBk, float* rowsum, long sRowsum, float* workspace, long workspace_bytes, long sBiasH, long sRowsumH,
                    int tasks, long sAt, long sBt, long sCt, long sBiasT, long sRowsumT);
/* which engine mtl_gemm_f32_ex / _tb picks (16-byte aligned operands, not transA && transB): 2 = bf16-split engine
 * (gemm_x3_kernel<...>, below -- also its split-K form: a product with fewer tiles than the engine's threshold and K >= 4096 that is
 * called with a workspace runs as equal K slices (batched launch into the workspace) + x3_splitk_sum_kernel, fixed order),
 * 1 = small-tile (gemm16_kernel<...>), 0 = forwarded to mtl_gemm_f32 (gemm_kernel<...>); used by bench.py to attribute launch
 * timings to the rocprofv3 kernel classes */
int mtl_gemm_f32_ex_route(int M, int N, int K, int batch, int kbatch, int has_rowsum);
/* Large products of mtl_gemm_f32_ex / _tb run on the bf16 matrix pipe: every fp32 operand element is split EXACTLY into three bf16
 * pieces on its way to LDS and a block product is six v_mfma_f32_32x32x16_bf16 accumulated in fp32 (a0 b0 + a0 b1 + a1 b0 + a1 b1 +
 * a0 b2 + a2 b0; dropped terms < 2^-23 |a||b|): fp32-class results (tests/test_ops_gpu.py compares both engines with fp64), no
 * scaling and no range caveat, 2.67 x the rate of the fp32 MFMA.  A product is routed there when its grid of 256 x 128 output tiles
 * (x batch items) has at least `min_tiles` workgroups and its operands are 16-byte aligned (csrc/mtl_gemm_x3.hip; nn.Linear forward
 * / backward of modules/common_layers.py:130,287-289,303 and modules/decoder.py:109 in a task-batched pass).
 * mtl_gemm_x3_min_tiles(set): set >= 0 replaces the threshold (0 = engine off; default 128 or the MTL_GEMM_X3 environment
 * variable), set < 0 only queries; returns the previous value. */
int mtl_gemm_x3_min_tiles(int set);

/* Task-batched two-piece fp16 product on the tile engine of csrc/mtl_gemm_x3.hip (256 x 128 x 32 tiles, 8 waves, split interleaved
 * with the MFMAs; 3 v_mfma_f32_32x32x16_f16 per step): for task t < tasks
 *   C_t[M,N] = A_t[M,K] . op(B_t) (+ bias_t[N]) (gate: C = gate_t[m][n] > 0 ? C : 0),   op(B) = B[N,K]^T (transB = 1) or B[K,N] (transB = 0),
 * operands of task t at base + t * s?t (sBt = 0: shared weights), its bounds max|A_t| / max|B_t| at amax_? + t * sAmax? floats
 * (MTL_AMAX_SLOTS slot heads each, as for the *_h2 convolutions; gate shares C's offsets).  The encoder's input Linear (5120 -> 512,
 * models/asr/transformer.py:136-140, modules/encoder.py:72) of all tasks of a pass in one launch, and its data gradient straight from the
 * un-transposed weight (transB = 0).  Any M, N, K; 16-byte aligned operands, lda / ldb / strides multiples of 4.
 * workspace (nullable): with ONE task, few output tiles and K >= 2048 the reduction is split over the grid into it (fixed-order sum). */
int mtl_gemm_h2_tb(void* stream, int transB, int M, int N, int K, const float* A, int lda, const float* amax_a, long sAmaxA,
                   const float* B, int ldb, const float* amax_b, long sAmaxB, float* C, int ldc, const float* bias, const float* gate,
                   int ldg, int tasks, long sAt, long sBt, long sCt, long sBiasT, float* workspace, long workspace_bytes);
/* the transposed-A form of the same engine: C_t[M,N] = A_t[K,M]^T . B_t[K,N] on two fp16 pieces (bounds as above) -- the weight gradient
 * of the encoder's input Linear, dW = de0^T . p2 (K = rows of the pass, M = 512, N = 5120), whose operands' bounds the pass has anyway */
int mtl_gemm_h2_tn_tb(void* stream, int M, int N, int K, const float* A, int lda, const float* amax_a, long sAmaxA, const float* B, int ldb,
                      const float* amax_b, long sAmaxB, float* C, int ldc, int tasks, long sAt, long sBt, long sCt);

/* ---- VGG front-end: models/asr/transformer.py:48-59 (Conv2d 3x3 s1 p1 + ReLU [+ MaxPool2d(2,2)]) ------
 * x_ref is the reference's (B,1,F,T) input; everything downstream is (B,T,F,C). */
/* amax_y (optional): MTL_AMAX_FLOATS floats, slot heads atomically raised to max(y) -- the `amax_x` of a following *_h2 convolution; zero them first. */
int mtl_conv0_relu_fwd(void* stream, const float* x_ref, const float* w /*(64,1,3,3)*/, const float* bias, float* y,
                       int B, int T, int F, float* amax_y);
long mtl_conv0_wgrad_workspace(void);
int mtl_conv0_wgrad(void* stream, const float* x_ref, const float* dy, float* dw /*accum*/, float* db /*accum*/,
                    float* workspace, int B, int T, int F);
/* conv0 and the conv bias column sums for the batches of `tasks` meta-tasks in one launch (pair) each -- the task-batched passes issue
 * them once per phase instead of once per task (8 launches of 8 samples: 593 / 527 / 132 us, one launch: 523 / 424 / 55 us).  Task k reads
 * its input batch at x + k sX floats (0: all tasks see the same batch, the shared validation batch), its weights / bias / output bound at
 * + k sW / sBias / sAmax floats; y and dy hold tasks * B samples; gradients accumulate onto dw + k sDw, db + k sDb.  Per task bitwise the
 * single-task calls for the forward; the weight gradient shares the 1024 partial rows of its workspace among the tasks. */
int mtl_conv0_relu_fwd_tb(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int T, int F, float* amax_y,
                          int tasks, long sX, long sW, long sBias, long sAmax);
int mtl_conv0_wgrad_tb(void* stream, const float* x, const float* dy, float* dw, float* db, float* workspace, int B, int T, int F, int tasks,
                       long sX, long sDw, long sDb);
/* the same four calls with C output channels: w (C,1,3,3), y / dy (B,T,F,C); C = 64 (vgg_cnn: exactly the calls above) or 32 (large_cnn,
 * models/asr/transformer.py:60-72).  Same workspace. */
int mtl_conv0c_relu_fwd(void* stream, const float* x_ref, const float* w, const float* bias, float* y, int B, int T, int F, int C,
                        float* amax_y);
int mtl_conv0c_wgrad(void* stream, const float* x_ref, const float* dy, float* dw /*accum*/, float* db /*accum*/, float* workspace, int B,
                     int T, int F, int C);
int mtl_conv0c_relu_fwd_tb(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int T, int F, int C,
                           float* amax_y, int tasks, long sX, long sW, long sBias, long sAmax);
int mtl_conv0c_wgrad_tb(void* stream, const float* x, const float* dy, float* dw, float* db, float* workspace, int B, int T, int F, int C,
                        int tasks, long sX, long sDw, long sDb);
/* column sums of `tasks` contiguous row blocks (rows x cols each) in one launch pair; workspace: tasks x mtl_colsum_workspace(rows, cols)
 * bytes (+ 16 per task); cols = 4 x 2^j <= 256, 16-byte aligned X */
int mtl_colsum_accum_tb(void* stream, const float* X, long rows, int cols, float* out, float* workspace, float* amax, int tasks, long sOut,
                        long sAmax);
/* (Cout,Cin,3,3) -> w_fwd [9][Cin][Cout] and w_dgrad [9][Cout][Cin] (taps rotated 180 degrees) */
int mtl_conv3x3_wprep(void* stream, const float* w_ref, float* w_fwd, float* w_dgrad, int Cout, int Cin);
int mtl_conv3x3_relu_fwd(void* stream, const float* x, const float* w_fwd, const float* bias, float* y, int B, int T,
                         int F, int Cin, int Cout);
/* fused conv + bias + ReLU + 2x2 max-pool (floor mode; first maximum in torch's window order wins):
 * p_out (B,T/2,F/2,Cout), argmax u8 in {0..3} = 2*(f&1) + (t&1).  The un-pooled activation is never written. */
int mtl_conv3x3_relu_pool_fwd(void* stream, const float* x, const float* w_fwd, const float* bias, float* p_out,
                              unsigned char* argmax, int B, int T, int F, int Cin, int Cout);
/* dx = conv_transpose(dy) gated by ReLU of the forward input activation `act` (same shape as dx).
 * argmax != NULL: dy is the POOLED gradient (B,T/2,F/2,Cout); un-pooling is fused into the operand load.
 * T,F,Cin,Cout describe the FORWARD convolution. */
int mtl_conv3x3_dgrad(void* stream, const float* dy, const unsigned char* argmax, const float* w_dgrad,
                      const float* act, float* dx, int B, int T, int F, int Cin, int Cout);
/* Split-bf16 ("x3") variants of the three calls above: identical semantics and fp32-class error, computed with six
 * v_mfma_f32_32x32x16_bf16 per 16-deep step on exact 3-way bf16 splits of both operands (2.67x the fp32 MFMA roof).
 * w3_fwd / w3_dgrad: bf16 [3][K-tile][rows][32] buffers (3 * 9*Cin*Cout * 2 bytes each) from mtl_conv3x3_wprep_x3; the four
 * 16-byte chunks of a row are stored at chunk ^ ((row >> 2) & 3) (the LDS image the kernels DMA with global_load_lds).
 * Shapes: Cin and Cout multiples of 64, and -- on the x3 calls only, single-task and _tb, weight gradients included -- the two narrow
 * layers of the large_cnn front-end, (Cin, Cout) = (32, 32) and (32, 64) (csrc/mtl_conv_narrow.hip).  Any other shape: MTL_EINVAL. */
int mtl_conv3x3_wprep_x3(void* stream, const float* w_ref, void* w3_fwd, void* w3_dgrad, int Cout, int Cin);
int mtl_conv3x3_relu_fwd_x3(void* stream, const float* x, const void* w3_fwd, const float* bias, float* y, int B, int T, int F,
                            int Cin, int Cout);
int mtl_conv3x3_relu_pool_fwd_x3(void* stream, const float* x, const void* w3_fwd, const float* bias, float* p_out,
                                 unsigned char* argmax, int B, int T, int F, int Cin, int Cout);
int mtl_conv3x3_dgrad_x3(void* stream, const float* dy, const unsigned char* argmax, const void* w3_dgrad, const float* act,
                         float* dx, int B, int T, int F, int Cin, int Cout);
/* Two-piece fp16 ("h2") variants: the same calls on 2-way fp16 splits of both operands -- three v_mfma_f32_32x32x16_f16 per
 * 16-deep step (half the matrix work of x3, twice its roof), fp32 accumulation, error ~1.5x that of an fp32 convolution
 * (h l' + l h' + h h' keeps 22 significand bits).  fp16 has 5 exponent bits, so every operand tensor comes with a DEVICE
 * BOUND `amax_*` >= max|tensor| (an upper bound within a few powers of two is as good): the kernels scale by the power of two
 * that puts the bound into [2^14, 2^15) before splitting and un-scale the accumulators exactly.  A bound is MTL_AMAX_FLOATS
 * floats: the maximum over its 64 slot heads counts (producers raise slot (workgroup % 64) atomically -- L2 serialises atomics
 * per cache line, one hot line costs thousands of them 40-300 us).  Producers deliver the bounds for free: `amax_y` / `amax_p` / `amax_dx` (optional outputs; zero all slots first),
 * mtl_conv0_relu_fwd's amax_y, mtl_colsum_accum's amax (the bias-gradient pass reads the whole gradient anyway; it WRITES all
 * slots), or mtl_absmax_f32.
 * w2_fwd / w2_dgrad: mtl_conv3x3_wprep_h2_bytes() each: [2][K-tile][rows][32] fp16 in the x3 layout + the fp32 weight scale. */
#ifndef MTL_AMAX_SLOTS
#define MTL_AMAX_SLOTS 64   /* every amax_* argument is MTL_AMAX_FLOATS floats: 64 slots, one 128-byte line apart (slot i at */
#define MTL_AMAX_STRIDE 32  /* [i * 32]); the bound is the maximum over the slot heads, the other floats are padding          */
#define MTL_AMAX_FLOATS (MTL_AMAX_SLOTS * MTL_AMAX_STRIDE)
#endif
long mtl_conv3x3_wprep_h2_bytes(int Cout, int Cin);
int mtl_conv3x3_wprep_h2(void* stream, const float* w_ref, void* w2_fwd, void* w2_dgrad, int Cout, int Cin);
/* the same for n <= 3 layers with one call (the pass prepares conv2 / conv5 / conv7 together); unused triples are ignored */
int mtl_conv3x3_wprep_h2_batch(void* stream, int n, const float* w0, void* f0, void* d0, int Cout0, int Cin0, const float* w1, void* f1,
                               void* d1, int Cout1, int Cin1, const float* w2, void* f2, void* d2, int Cout2, int Cin2);
/* ... and for `sets` parameter sets (the theta' stack of a task-batched validation pass) with the same two launches: set z reads its
 * weights at w_i + z sSrc floats and writes its prepared blocks at f_i / d_i + z sDst_i BYTES (multiples of 4) */
int mtl_conv3x3_wprep_h2_batch_tb(void* stream, int n, const float* w0, void* f0, void* d0, int Cout0, int Cin0, const float* w1, void* f1,
                                  void* d1, int Cout1, int Cin1, const float* w2, void* f2, void* d2, int Cout2, int Cin2, int sets,
                                  long sSrc, long sDst0, long sDst1, long sDst2);
int mtl_conv3x3_relu_fwd_h2(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* y,
                            float* amax_y, int B, int T, int F, int Cin, int Cout);
int mtl_conv3x3_relu_pool_fwd_h2(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias,
                                 float* p_out, unsigned char* argmax, float* amax_p, int B, int T, int F, int Cin, int Cout);
int mtl_conv3x3_dgrad_h2(void* stream, const float* dy, const float* amax_dy, const unsigned char* argmax, const void* w2_dgrad,
                         const float* act, float* dx, float* amax_dx, int B, int T, int F, int Cin, int Cout);
/* The same three launches for the batches of `tasks` meta-tasks at once (trainer/asr/transient_trainer.py:178-237: the tasks of a
 * meta-step are independent given theta0): x / y / dy / dx / act / argmax hold tasks * B samples, task k = samples [k B, (k + 1) B);
 * task k reads its prepared weights at w2 + k * sW BYTES (0: all tasks share theta0's -- the training passes), its bias at
 * bias + k * sBias floats, its operand bound at amax + k * sAmaxX floats and raises its own output bound at amax_y + k * sAmaxY.
 * Per task bitwise the single-task launch (same tiles, same scales); one launch of 64 samples costs 2-14 % less than eight of 8.
 * widths (optional, `tasks` ints on the device, with mtl_zero_tails): the tasks' own frame counts when their batches were stacked at a
 * common T; rows t >= widths[k] >> wshift of task k's samples (t = the row index of this launch's convolution: before its pooling, the
 * data gradient's output rows) are then NOT computed -- whole pixel-tile rows beyond them are left out of the launch and their outputs
 * stay untouched: the caller clears them (mtl_zero_tails) before anything reads them.  NULL: every row. */
int mtl_conv3x3_relu_fwd_h2_tb(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* y,
                               float* amax_y, int B, int T, int F, int Cin, int Cout, int tasks, long sW, long sBias, long sAmaxX, long sAmaxY,
                               const int* widths, int wshift);
int mtl_conv3x3_relu_pool_fwd_h2_tb(void* stream, const float* x, const float* amax_x, const void* w2_fwd, const float* bias, float* p_out,
                                    unsigned char* argmax, float* amax_p, int B, int T, int F, int Cin, int Cout, int tasks, long sW,
                                    long sBias, long sAmaxX, long sAmaxP, const int* widths, int wshift);
int mtl_conv3x3_dgrad_h2_tb(void* stream, const float* dy, const float* amax_dy, const unsigned char* argmax, const void* w2_dgrad,
                            const float* act, float* dx, float* amax_dx, int B, int T, int F, int Cin, int Cout, int tasks, long sW,
                            long sAmaxDy, long sAmaxDx, const int* widths, int wshift);
/* weight (+ bias) gradients of `tasks` meta-tasks in one launch: x / dy / argmax hold tasks * B samples; task k reads its bounds at
 * amax_x + k sAmaxX, amax_dy + k sAmaxDy floats and accumulates onto dw_ref + k sDw, db + k sDb floats (the per-task gradient stack).
 * The launch's partial slabs (workspace: mtl_conv3x3_wgrad_x3_workspace, unchanged) are dealt to the tasks in equal contiguous ranges,
 * so one launch writes / reduces as many slabs as ONE single-task launch; tasks <= slabs.  Fixed-order sums: deterministic; the
 * partition of a task's pixels over slabs differs from the single-task launch (same class of rounding, not the same bits). */
int mtl_conv3x3_wgrad_h2_tb(void* stream, const float* x, const float* amax_x, const float* dy, const float* amax_dy,
                            const unsigned char* argmax, float* dw_ref, float* db, float* workspace, long workspace_bytes, int B, int T,
                            int F, int Cin, int Cout, int tasks, long sAmaxX, long sAmaxDy, long sDw, long sDb);
/* The same four several-task launches on the EXACT 3 x bf16 split (MTL_CONV=x3: every fp32 operand bit kept, models/asr/transformer.py:48-59
 * is fp32): no bounds; w3 + k * sW bytes, bias + k * sBias floats, dw_ref + k sDw / db + k sDb floats as above (db nullable: the bias
 * gradient = per-channel sums of dy rides on the weight-gradient launch). */
int mtl_conv3x3_relu_fwd_x3_tb(void* stream, const float* x, const void* w3_fwd, const float* bias, float* y, int B, int T, int F, int Cin,
                               int Cout, int tasks, long sW, long sBias, const int* widths, int wshift);
int mtl_conv3x3_relu_pool_fwd_x3_tb(void* stream, const float* x, const void* w3_fwd, const float* bias, float* p_out, unsigned char* argmax,
                                    int B, int T, int F, int Cin, int Cout, int tasks, long sW, long sBias, const int* widths, int wshift);
int mtl_conv3x3_dgrad_x3_tb(void* stream, const float* dy, const unsigned char* argmax, const void* w3_dgrad, const float* act, float* dx,
                            int B, int T, int F, int Cin, int Cout, int tasks, long sW, const int* widths, int wshift);
int mtl_conv3x3_wgrad_x3_tb(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref, float* db,
                            float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout, int tasks, long sDw, long sDb);
/* amax[MTL_AMAX_FLOATS]: slot heads raised so that their maximum is >= max|x[0..n)| (atomic; zero them first) */
int mtl_absmax_f32(void* stream, const float* x, long n, float* amax);
/* the same for `tasks` tensors of n floats at x + k sX, bound k at amax + k sAmax floats, one launch */
int mtl_absmax_f32_tb(void* stream, const float* x, long n, float* amax, int tasks, long sX, long sAmax);
/* Census of an h2 operand against its bound -- the runtime guard of the two-piece fp16 arithmetic (csrc/mtl_h2.h: one power-of-two scale per
 * tensor; an element more than ~2^17.5 below max|tensor| keeps fewer than 22 significand bits).  For `tasks` tensors of n floats at
 * x + k sX with bounds at amax + k sAmax floats, ADDS to counts + k sCounts (three 64-bit counters each; zero them first):
 * [0] non-zero elements, [1] of those, elements that keep fewer than 22 bits, [2] fewer than 16 bits.  Exact (integer atomics).
 * The reference's inputs are normalised per utterance (utils/data_loader.py:84-94), which is why its activations stay in the
 * full-precision regime; TransientTrainer samples this census periodically and leaves h2 when they do not. */
int mtl_h2_census(void* stream, const float* x, long n, const float* amax, unsigned long long* counts, int tasks, long sX, long sAmax,
                  long sCounts);
/* Several tasks' batches of different frame counts in ONE pass, padded to the widest (data.py collate pads every task's batch to its OWN
 * longest utterance, transient_trainer.py:178-237 runs them one by one): y is (n, T, row) floats, sample s belongs to task s / per_task and
 * its frames [widths[task] >> shift, T) are cleared, so that the next convolution meets the zero border of the task's own image and the
 * ReLU gates of the backward hold every gradient out of them.  widths: `n / per_task` ints on the device (full-resolution frame counts;
 * shift = 1 after the first pooling).  row % 4 == 0, y 16-byte aligned. */
int mtl_zero_tails(void* stream, float* y, int n, int T, int row, const int* widths, int shift, int per_task);
long mtl_conv3x3_wgrad_workspace(int B, int T, int F, int Cin, int Cout, int pooled);
/* dw_ref (Cout,Cin,3,3) += sum_pixels x (x) dy ; dy dense (B,T,F,Cout) or pooled + argmax as above. */
int mtl_conv3x3_wgrad(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref,
                      float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout);
/* Split-bf16 ("x3") weight gradient: same contract as the two calls above (its own workspace size).  Halo-tiled x staged in
 * LDS, transpose reads (ds_read_b64_tr_b16) for the pixel-major reduction, dy fragments loaded straight into MFMA layout. */
long mtl_conv3x3_wgrad_x3_workspace(int B, int T, int F, int Cin, int Cout, int pooled);
int mtl_conv3x3_wgrad_x3(void* stream, const float* x, const float* dy, const unsigned char* argmax, float* dw_ref,
                         float* workspace, long workspace_bytes, int B, int T, int F, int Cin, int Cout);
/* h2 weight gradient (workspace: mtl_conv3x3_wgrad_x3_workspace); amax_dy bounds the dense OR the pooled gradient it is given.
 * db (nullable, accum): the bias gradient db[c] += sum over pixels of dy -- the kernel's dy loaders see every element anyway, so
 * the separate column-sum pass over dy (164 MB for conv5) is not needed. */
int mtl_conv3x3_wgrad_h2(void* stream, const float* x, const float* amax_x, const float* dy, const float* amax_dy,
                         const unsigned char* argmax, float* dw_ref, float* db, float* workspace, long workspace_bytes, int B, int T,
                         int F, int Cin, int Cout);
/* wp[o][h*C+c] = w[o][c*Hh+h]  (inverse_accum: dst[o][c*Hh+h] += src[o][h*C+c]); the (C*H) flattening of
 * models/asr/transformer.py:136-138 folded into encoder.input_linear's weight instead of an activation copy. */
int mtl_permute_hc(void* stream, const float* src, float* dst, int rows, int C, int Hh, int inverse_accum,
                   float* amax /* nullable, MTL_AMAX_FLOATS: raised to max|src| (zero it first) */);
/* the same for `tasks` weight sets at strides sSrc / sDst (floats) and bounds at sAmax (floats) in ONE launch (the theta' stack) */
int mtl_permute_hc_tb(void* stream, const float* src, float* dst, int rows, int C, int Hh, int inverse_accum, float* amax, int tasks,
                      long sSrc, long sDst, long sAmax);

/* ---- LayerNorm(x + residual) * gamma + beta (+ pe[row % T]) then * keep[row] -----------------------------
 * nn.LayerNorm eps inside the sqrt, biased variance (modules/common_layers.py:131,304; modules/encoder.py:72-73)
 * with the non_pad_mask multiplies of modules/encoder.py:101,104 and modules/decoder.py:314,318,321 fused.
 * d in {64,128,256,512,1024}.  Saves xhat (rows x d) and rstd (rows) for the backward. */
/* xmask (nullable u8 keep-mask of x, from mtl_dropout_mask) / xscale = 1/(1-p): dropout of the sub-layer output BEFORE the
 * residual add (modules/common_layers.py:130,303). */
int mtl_layernorm_fwd(void* stream, const float* x, const float* residual, const float* gamma, const float* beta,
                      const float* pe, const int* keep, const unsigned char* xmask, float xscale, float* y, float* xhat,
                      float* rstd, int rows, int d, int T, float eps);
/* Task-grouped form: the rows are consecutive groups of rows_per_group rows (the batches of the tasks of a meta-step in one
 * launch); group g reads gamma / beta at + g * sParam floats (0: shared parameters). */
int mtl_layernorm_fwd_g(void* stream, const float* x, const float* residual, const float* gamma, const float* beta,
                        const float* pe, const int* keep, const unsigned char* xmask, float xscale, float* y, float* xhat,
                        float* rstd, int rows, int d, int T, float eps, int rows_per_group, long sParam);
long mtl_layernorm_bwd_workspace(int rows, int d);
/* with xmask: dz is the residual-branch gradient and dzm = dz * mask * xscale the sub-layer-branch gradient (dsum sums dzm);
 * dz2 (nullable): a second copy of dz (the residual path accumulates onto it while dz stays intact for the weight gradient) */
int mtl_layernorm_bwd(void* stream, const float* dy, const float* xhat, const float* rstd, const float* gamma,
                      const int* keep, const unsigned char* xmask, float xscale, float* dz, float* dzm /*nullable*/,
                      float* dz2 /*nullable*/, float* dgamma /*accum*/, float* dbeta /*accum*/,
                      float* dsum /*nullable, accum: += column sums of the sub-layer-branch gradient (its linear's bias grad)*/,
                      float* workspace, int rows, int d,
                      int defer_reduce /* 1: leave the per-wave partials in `workspace` (keep it alive, one per instance) and add them
                                          to dgamma / dbeta / dsum later with mtl_ln_param_reduce_batch */);
/* Task-grouped form: a wave's rows belong to one group; group g owns the partial rows [g * W, (g + 1) * W) of `workspace`
 * (W = mtl_layernorm_bwd_g_waves(rows_per_group); 3 * d floats per partial row), reads gamma at + g * sParam and -- unless the
 * reduction is deferred -- adds to dgamma / dbeta / dsum at + g * sGrad. */
int mtl_layernorm_bwd_g_waves(int rows_per_group);
long mtl_layernorm_bwd_g_workspace(int rows, int d, int rows_per_group);
int mtl_layernorm_bwd_g(void* stream, const float* dy, const float* xhat, const float* rstd, const float* gamma,
                        const int* keep, const unsigned char* xmask, float xscale, float* dz, float* dzm, float* dz2, float* dgamma,
                        float* dbeta, float* dsum, float* workspace, int rows, int d, int defer_reduce, int rows_per_group,
                        long sParam, long sGrad);
/* the deferred parameter reductions of several mtl_layernorm_bwd calls in ONE launch (table in device memory; nw = workspace bytes
 * / (3 * d * 4); dmax = largest d of the table) */
typedef struct mtl_ln_reduce_desc {
    const float* part;
    float* dgamma;
    float* dbeta;
    float* dsum; /* nullable */
    int nw, d;
} mtl_ln_reduce_desc;
int mtl_ln_param_reduce_batch(void* stream, const mtl_ln_reduce_desc* table_dev, int n, int dmax);

/* ---- masked softmax: modules/common_layers.py:322-327.  S is [B][H][Tq][ld], in place.
 * keys k >= klen[b] (klen nullable) and, if causal, k > q are filled with -inf before the softmax.
 * A row without a live key (klen[b] <= 0) becomes all zeros, not the NaN torch.softmax gives for an all -inf row; its backward is zero too. */
/* pmask (nullable u8 keep-mask, same [B][H][Tq][ld] layout) / pscale: dropout on the probabilities (common_layers.py:328);
 * P stays un-dropped in S (needed by the backward), the dropped copy that feeds P.V is written to P_dropped. */
int mtl_softmax_mask_fwd(void* stream, float* S, const int* klen, int causal, float scale, int B, int H, int Tq, int Tk,
                         int ld, const unsigned char* pmask, float pscale, float* P_dropped);
int mtl_softmax_bwd(void* stream, const float* P, float* dP /*in place -> dS*/, float scale, long rows, int Tk, int ld,
                    const unsigned char* pmask, float pscale);

/* ---- fused scaled-dot-product attention: modules/common_layers.py:317-331 (bmm, /temperature, masked_fill(-inf), softmax,
 * dropout, bmm) with the head split / merge of :291-293,301 done by stride and the masks of :296 derived in-kernel.
 * q (B*Tq rows, row stride ldq floats), k, v (B*Tk rows): head h occupies columns [h*dk, (h+1)*dk) of a row (dv for v / O).
 * keys k >= klen[b] (klen nullable) and, if causal, k > q are masked.  O (B*Tq rows, ldo) = softmax(q.k^T * scale) [* pmask *
 * pscale] . v ; lse[(b*H+h)*Tq + q] = log-sum-exp of the scaled scores (saved for the backward).  The (B,H,Tq,Tk) score tensor
 * is never written: 64-query workgroups stream 64-key tiles with an online softmax; the backward recomputes the probabilities.
 * pmask (nullable): u8 keep-mask [B][H][Tq][ldm] from mtl_dropout_mask, pscale = 1/(1-p).  (dk, dv) in {(64,64), (16,16)}
 * (mtl_attn_supported); q/k/v/dO 16-byte aligned with row strides that are multiples of 4.
 * Backward: dq, dk, dv are OVERWRITTEN (head-strided like their inputs); delta: B*H*Tq floats of scratch. */
int mtl_attn_supported(int dk, int dv);
int mtl_attn_fwd(void* stream, const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const int* klen,
                 int causal, float scale, int B, int H, int Tq, int Tk, int dk, int dv, const unsigned char* pmask, int ldm,
                 float pscale, float* O, int ldo, float* lse);
int mtl_attn_bwd(void* stream, const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const int* klen,
                 int causal, float scale, int B, int H, int Tq, int Tk, int dk, int dv, const unsigned char* pmask, int ldm,
                 float pscale, const float* O, const float* dO, int ldo, const float* lse, float* delta, float* dq, float* dk_,
                 float* dv_, int lddq, int lddk, int lddv);

/* ---- the middle of the factorized feed-forward block (--is-factorized; modules/common_layers.py:134-158) as one streamed kernel
 * (csrc/mtl_ffn_lr.hip):  h = relu(a . B1^T + b1),  c = h . A2^T  with a (rows x r, row stride lda) the output of linear_1_a,
 * B1 = linear_1_b.weight (inner x r), b1 its bias (inner), A2 = linear_2_a.weight (r x inner), c (rows x r, row stride ldc) the input
 * of linear_2_b.  h (nullable; rows x inner, dense) receives the post-ReLU activation for the backward; c is bitwise the same with
 * and without it.  `rows` is per task: task t < tasks reads a + t * sAt, the three weights + t * sWt floats (0: all tasks share
 * them), and writes h + t * sHt, c + t * sCt.  Any rows >= 1; r a multiple of 4 up to 128 and inner a multiple of 4
 * (mtl_ffn_lr_mid_supported; MTL_EINVAL otherwise); a, B1, A2 16-byte aligned, lda / sAt / sWt multiples of 4.  Exact bf16 triples,
 * six MFMAs per block product, fixed summation order (bitwise reproducible), no atomics, no workspace. */
int mtl_ffn_lr_mid_supported(int r, int inner);
int mtl_ffn_lr_mid_fwd(void* stream, const float* a, int lda, const float* B1, const float* b1, const float* A2, float* h, float* c,
                       int ldc, int rows, int r, int inner, int tasks, long sAt, long sWt, long sHt, long sCt);

/* ---- the encoder's input Linear of a model without a convolutional front-end (feat_extractor 'none'; csrc/mtl_featproj.hip) on the
 * feature planes as the batch brings them and the weight as nn.Linear stores it:
 *   y[(b T + p), n] = bias[n] + sum_f x[b, f, p] w[n, f]        for every sample b < B and frame p < T of every task
 * x (B, F, T) fp32 planes, w (N, F) row-major, bias (N; nullable), y (B T, N) dense.  Task t < tasks reads x + t * sX (0: all tasks
 * share one batch), w and bias + t * sW (0: all tasks share the parameters; the two stand in one parameter buffer), writes
 * y + t * sY (floats).  Any F, T, N >= 1; NO alignment is asked of any operand or row, and nothing is read past an operand's end.
 * Exact bf16 triples, six MFMAs per block product, fixed order: bitwise reproducible, and a task's result does not depend on `tasks`.
 * MTL_EINVAL before any launch for null operands (bias excepted), non-positive extents, negative strides, B or tasks > 65535. */
int mtl_featproj_fwd_tb(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int F, int T, int N,
                        int tasks, long sX, long sW, long sY);
/* its weight gradient  dw_t[n, f] += sum_{b, p} dy_t[(b T + p), n] x_t[b, f, p]  (dy dense (B T, N), task stride sDy; dw at task stride
 * sG floats, >= N F when tasks > 1).  The B T rows are split over the grid into `workspace` (mtl_featproj_wgrad_workspace bytes; the
 * split depends on B T, F and N alone, never on `tasks`) and summed in a fixed order: no atomics, bitwise reproducible, per task bitwise the one-task launch.
 * MTL_EINVAL as above, and for a null or too small workspace. */
long mtl_featproj_wgrad_workspace(int B, int F, int T, int N, int tasks);
int mtl_featproj_wgrad_tb(void* stream, const float* x, const float* dy, float* dw, float* workspace, long workspace_bytes, int B,
                          int F, int T, int N, int tasks, long sX, long sDy, long sG);

/* ---- embedding + positional encoding: modules/decoder.py:96 ------------------------------------------- */
int mtl_embed_pe_fwd(void* stream, const long* ids, const float* table, const float* pe, float* out, int rows, int T, int d,
                     const unsigned char* mask /*nullable: dropout keep-mask*/, float mscale);
/* first[r] = 1 if no earlier row has ids[r]; next[r] = next row with the same id or -1 (both host-built): duplicates are
 * summed in row order by the thread of the chain head, so the scatter-add is one launch, parallel AND deterministic. */
int mtl_embed_bwd(void* stream, const long* ids, const int* first, const int* next, const float* dout,
                  float* dtable /*accum*/, int rows, int d, long pad_id, const unsigned char* mask, float mscale);

/* Task-grouped forms: rows in groups of rows_per_group; group g uses table + g * sParam / dtable + g * sGrad.  The occurrence
 * chains (first / next) must not cross groups. */
int mtl_embed_pe_fwd_g(void* stream, const long* ids, const float* table, const float* pe, float* out, int rows, int T, int d,
                       const unsigned char* mask, float mscale, int rows_per_group, long sParam);
int mtl_embed_bwd_g(void* stream, const long* ids, const int* first, const int* next, const float* dout, float* dtable, int rows,
                    int d, long pad_id, const unsigned char* mask, float mscale, int rows_per_group, long sGrad);

/* ---- dropout keep-masks: keep[i] = 1 with probability 1-p, Philox4x32-10(counter = offset + i/4, key = *seed_dev).
 * Active sites in the meta loop (model.train()): modules/decoder.py:96, modules/common_layers.py:130,303,328. */
int mtl_dropout_mask(void* stream, unsigned char* keep, long n, float p, const long* seed_dev, unsigned long long offset);

/* ---- cross-entropy + arg-max: utils/metrics.py:113-126, models/asr/transformer.py:146-147 ----------------
 * loss_out[0] = sum_rows(gold!=pad ? -log softmax(logits)[gold] : 0) / n_nonpad ; hyp = lowest arg-max index. */
/* inv_count_dev (nullable): device scalar 1/n_nonpad used instead of n_nonpad (keeps a captured hipGraph batch-independent) */
int mtl_ce_argmax_fwd(void* stream, const float* logits, const long* gold, int rows, int V, int ld, long pad_id,
                      float smoothing, int n_nonpad, const float* inv_count_dev, float* lse, long* hyp, float* rowloss,
                      float* loss_out);
/* dlogits = gscale * (gscale_dev ? *gscale_dev : 1) * (softmax - target) on non-pad rows, 0 elsewhere */
int mtl_ce_bwd(void* stream, const float* logits, const float* lse, const long* gold, int rows, int V, int ld, long pad_id,
               float smoothing, float gscale, const float* gscale_dev, float* dlogits, int ldd);

/* Task-grouped forms (rows % rows_per_group == 0): loss_out[g] = sum over the rows of group g * inv_count_dev[g] (one loss per
 * task, each normalised by ITS non-pad token count); the backward scales group g by gscale * gscale_dev[g]. */
int mtl_ce_argmax_fwd_g(void* stream, const float* logits, const long* gold, int rows, int V, int ld, long pad_id, float smoothing,
                        const float* inv_count_dev, float* lse, long* hyp, float* rowloss, float* loss_out, int rows_per_group);
int mtl_ce_bwd_g(void* stream, const float* logits, const float* lse, const long* gold, int rows, int V, int ld, long pad_id,
                 float smoothing, float gscale, const float* gscale_dev, float* dlogits, int ldd, int rows_per_group);

/* ---- out[c] += sum_r X[r*ld + c]  (bias gradients) -------------------------------------------------------- */
long mtl_colsum_workspace(long rows, int cols);
/* amax (optional, MTL_AMAX_FLOATS floats): all slot heads set to max|X| (written, not accumulated) -- the same pass over X */
int mtl_colsum_accum(void* stream, const float* X, long rows, int cols, long ld, float* out, float* workspace, float* amax);

/* ---- flat-parameter updates over ONE contiguous fp32 buffer (190 tensors in the reference) ----------------
 * inner SGD  trainer/asr/transient_trainer.py:106,207 -> theta1 = theta0 - alpha*g (theta0 is never mutated, which
 *            replaces deepcopy(state_dict)/load_state_dict at :155-160,237)
 * copy_grad  models/asr/transformer.py:205-240       -> mtl_axpy(G, g, 1)
 * clip       transient_trainer.py:205-206,253-254     -> mtl_sumsq(mode 2) + mtl_scale(a_dev)
 * Adam       transient_trainer.py:109,255 (torch defaults) */
int mtl_sgd_theta_prime(void* stream, const float* theta0, const float* g, float alpha, float* theta1, long n);
/* the inner steps of all local tasks in one launch: theta1[t*n + i] = theta0[i] - alpha * g[t*n + i], t < tasks (n % 4 == 0) */
int mtl_sgd_theta_prime_tasks(void* stream, const float* theta0, const float* g, float alpha, float* theta1, long n, int tasks);
/* out[i] (+)= sum_t x[t*n + i] in task order (copy_grad accumulation of a task stack: models/asr/transformer.py:219-229) */
int mtl_sum_tasks(void* stream, float* out, const float* x, long n, int tasks, int accumulate);
/* the same over a SLICE of the stack: out[i] (+)= sum_t x[t*task_stride + i], i < n (n, task_stride % 4 == 0, 16-byte aligned): one
 * parameter group (decoder | encoder | conv) of copy_grad as soon as its gradients are final, so that its all-reduce can start under
 * the rest of the backward (trainer/asr/transient_trainer.py:229,247-255) */
int mtl_sum_tasks_strided(void* stream, float* out, const float* x, long n, int tasks, long task_stride, int accumulate);
int mtl_axpy(void* stream, float* y, const float* x, float a, long n);
int mtl_copy_f32(void* stream, float* dst, const float* src, long n); /* device-to-device, asynchronous on `stream` */
int mtl_scale(void* stream, float* y, float a, const float* a_dev /*nullable: overrides a*/, long n);
int mtl_adam_step(void* stream, float* theta, const float* G, float* m, float* v, int step, float lr, float beta1,
                  float beta2, float eps, long n);
int mtl_sumsq(void* stream, const float* x, long n, float* out, float* workspace /* >= 4 KiB */, int mode, float arg);
/* the clipped SGD step of the LM epoch loops (lm/main.py:273-277) in ONE pass over both buffers: theta becomes, bit for bit, what
 * mtl_scale(g, 1, coef_dev, n) followed by mtl_axpy(theta, g, -lr, n) leaves (coef_dev NULL: coefficient 1; the product coef * g is
 * rounded to fp32 before the update), g is set to zero, and -- when both pointers are given -- loss_acc[0] += loss[0] in fp32 by one
 * thread.  theta, g 16-byte aligned, any n >= 1.  -22 for a null theta or g, n < 1 or a misaligned buffer. */
int mtl_sgd_clip_step(void* stream, float* theta, float* g, float lr, const float* coef_dev, long n, const float* loss, float* loss_acc);

/* ---- spectrogram front-end (utils/data_loader.py:65-96): after the STFT has been computed as
 * mtl_gemm_f32(frames (T x n_fft, lda = hop: overlapping rows of the padded waveform) . windowed DFT basis (n_fft x 2F)),
 * out[f*T + t] = log1p(|X[t][f]|), optionally followed by (x - mean) / std (unbiased) over the whole utterance.
 * partials: >= 256 doubles of scratch. */
int mtl_spect_logmag(void* stream, const float* reim, int ld, int T, int F, float* out, double* partials, int normalize);
/* The whole front-end for a sampled batch of K utterances in two launches (csrc/mtl_spect.hip; utils/data_loader.py:65-96 per utterance,
 * and the zero-padded (K, 1, F, Tmax) batch of :284-297): framing, STFT, |.|, log1p, per-utterance (x - mean) / std and the padding.
 *   wav: the K waveforms concatenated; offsets: K + 1 int64, utterance k = wav[offsets[k] .. offsets[k+1]), L_k samples, T_k = 1 + L_k / hop
 *   frames.  Sample n of frame t is index t hop + n - n_fft/2 of the utterance, reflected once at either end (center=True,
 *   pad_mode='reflect'): L_k >= n_fft/2 + 1 is the CALLER's promise (the offsets live on the device; the kernel clamps, it cannot refuse).
 *   basis: n_fft x ldb, [w cos | -w sin] (F columns each), ldb >= 2 F.  n_fft even and <= 1024, hop >= 1, F = n_fft/2 + 1, 1 <= K <= 2^20, Tmax >= 1.
 *   out (K, F, Tmax): out[k][f][t] = log1p|X_k[t][f]| for t < min(T_k, Tmax), normalised when `normalize` with the mean / unbiased std over
 *   ALL F T_k values of the utterance (frames beyond Tmax count), and exactly 0 for min(T_k, Tmax) <= t < Tmax.
 * The frames are formed inside the kernel from an LDS-staged span of samples (no padded copy, no frame matrix in memory), the product
 * runs on v_mfma_f32_16x16x4_f32, the statistics are fp64 partials combined in a fixed order: bitwise repeatable, no atomics.  The
 * number of launches (2) and the grid do not depend on the lengths.  workspace: mtl_spect_batch_workspace(sum of T_k, K, F) bytes,
 * 8-byte aligned. */
long mtl_spect_batch_workspace(long total_frames, int K, int F);
int mtl_spect_batch(void* stream, const float* wav, const long* offsets, int K, int n_fft, int hop, const float* basis, int ldb, int F,
                    float* out, int Tmax, int normalize, void* workspace, long workspace_bytes);
/* Noise injection on the device (NoiseInjection.inject_noise_sample, utils/data_loader.py:383-399: data += level * noise *
 * rms(data) / rms(noise), noise = a segment of a noise file as long as the utterance).  The noise corpus is ONE int16 bank of bank_len
 * samples resident on the device; utterance k (wav / offsets as in mtl_spect_batch, n = L_k samples) takes bank[noise_off[k] .. + n),
 * noise_off[k] < 0 = clean.  Every bank address is clamped into [0, bank_len): a wrong table cannot read out of bounds.
 *   mtl_wave_mix_coef (utils/data_loader.py:383-399, the two energies of :396-397): coef[k] = (float)(level[k] sqrt(S_d / n) /
 *     sqrt(S_n / n)) formed in fp64, S_d = sum data^2, S_n = sum noise^2 with noise = (float)int16 / 32768 (exact), fp64 partial sums
 *     combined in a fixed order (no atomics: bitwise repeatable); coef[k] = 0 for noise_off[k] < 0 and for S_n == 0.
 *     workspace: mtl_wave_mix_coef_workspace(K) bytes, 8-byte aligned. */
long mtl_wave_mix_coef_workspace(int K);
int mtl_wave_mix_coef(void* stream, const float* wav, const long* offsets, int K, const short* bank, long bank_len, const long* noise_off,
                      const float* level, float* coef, void* workspace, long workspace_bytes);
/*   mtl_wave_mix (utils/data_loader.py:383-399, the sum of :398): out[offsets[k] + i] = fmaf(coef[k], noise_i, wav[offsets[k] + i]) in
 *     fp32 for the K packed waveforms (out has the layout of wav); coef[k] == 0 or noise_off[k] < 0 copies the utterance bit for bit. */
int mtl_wave_mix(void* stream, const float* wav, const long* offsets, int K, const short* bank, long bank_len, const long* noise_off,
                 const float* coef, float* out);
/*   mtl_spect_batch_noise (utils/data_loader.py:383-399 in front of :65-96): mtl_spect_batch of the MIXED waveforms without forming them
 *     in memory -- the same kernel, the staged sample being the expression of mtl_wave_mix at the (reflected) index, so the result is
 *     bitwise that of mtl_spect_batch on mtl_wave_mix's output.  A workgroup of an utterance with coef 0 does not read the bank. */
int mtl_spect_batch_noise(void* stream, const float* wav, const long* offsets, int K, int n_fft, int hop, const float* basis, int ldb, int F,
                          float* out, int Tmax, int normalize, void* workspace, long workspace_bytes, const short* bank, long bank_len,
                          const long* noise_off, const float* coef);
/* Tempo and gain augmentation on the device (load_randomly_augmented_audio, utils/audio.py:35-61: `sox tempo f gain g` into a 16-bit
 * file), in front of the calls above (csrc/mtl_tempo.hip).  sox is not reproduced sample for sample (it dithers): the behaviour is DEFINED
 * here and in DESIGN.md section 12, parity unpinned.  wav / offsets as in mtl_spect_batch (utterance k: L_k samples, read as 0 at and
 * beyond L_k); out_offsets: K + 1 int64, the stretched utterance k has N_k = out_offsets[k+1] - out_offsets[k] samples (the caller's
 * N_k = floor(L_k / f_k + 0.5), or L_k for f_k == 1); tempo: K doubles f_k.  WSOLA with segment `seg`, search `search`, overlap `overlap`
 * samples (1 <= overlap <= 256, 0 <= search <= 255, seg > overlap), H = seg - overlap: M_k = ceil(N_k / H) segments, segment m starts at
 * p_m = floor(f (m H) + 0.5) (IEEE fp64, one multiply, one add) shifted by o_m in [0, search]; o_0 = search / 2, o_m = the c that
 * minimises sum_{i < overlap} (tail_{m-1}[i] - x[p_m + c + i])^2, tail_{m-1}[i] = x[p_{m-1} + o_{m-1} + H + i], fp64 sums in index order,
 * the smallest c on a tie.  seg_base: K + 1 int64, utterance k owns seg_off[seg_base[k] .. seg_base[k+1]) (>= M_k entries; f_k == 1.0:
 * the effect is bypassed, none are written or read).  1 <= K <= 2^20.  No workspace, no atomics: bitwise repeatable.
 *   mtl_tempo_search: seg_off[seg_base[k] + m] = o_m.  One workgroup per utterance walks the chain (tail_m depends on o_m). */
int mtl_tempo_search(void* stream, const float* wav, const long* offsets, const long* out_offsets, const double* tempo, const long* seg_base,
                     int K, int seg, int search, int overlap, int* seg_off);
/*   mtl_tempo_render: out[out_offsets[k] + m H + i] (i < H) = x[p_m + o_m + i], and for m >= 1, i < overlap the cross-fade
 *     fmaf(i / overlap, x[p_m + o_m + i] - tail_{m-1}[i], tail_{m-1}[i]) in fp32; f_k == 1.0 copies.  quantize != 0: every sample t then
 *     becomes clip(rint(t gain[k] 32768), -32768, 32767) / 32768 (gain: K floats, linear; the 16-bit file without dither);
 *     quantize == 0: the raw overlap-add, gain (nullable) is not read.  Table entries are clamped into [0, search]: a wrong table
 *     cannot read out of bounds.  out has sum of N_k floats. */
int mtl_tempo_render(void* stream, const float* wav, const long* offsets, const long* out_offsets, const double* tempo, const float* gain,
                     const long* seg_base, const int* seg_off, int K, int seg, int search, int overlap, int quantize, float* out);
/* Sample-rate conversion on the device (audio_with_sox / augment_audio_with_sox, utils/audio.py: `sox -r`), in front of the tempo calls
 * (csrc/mtl_resample.hip).  sox is not reproduced sample for sample: the behaviour is DEFINED here and in DESIGN.md section 14, parity
 * unpinned.  wav / offsets as in mtl_spect_batch (utterance k: L_k samples, read as 0 outside [0, L_k)); out_offsets: K + 1 int64, the
 * converted utterance k has N_k = out_offsets[k+1] - out_offsets[k] samples (the caller's N_k = ceil(L_k up_k / down_k)).
 *   plan: 4 int64 per utterance: up_k, down_k, half_k and base_k, its filter being taps[base_k .. base_k + 2 half_k] (n_taps doubles in
 *   all, the filters of the distinct ratios one after the other; formed by the caller in fp64 and used as uploaded).
 *   out[out_offsets[k] + j] = sum_i x[i] taps[base_k + j down_k - i up_k + half_k] over 0 <= i < L_k with the tap index in
 *   [0, 2 half_k]: fp64, one fma per term, ascending i; j down_k and every offset are 64-bit.  up_k == down_k copies the utterance bit
 *   for bit.  quantize != 0: every converted sample y then becomes clip(rint(y 32768), -32768, 32767) / 32768, formed in fp64 (the
 *   16-bit file without dither; the copies of the bypass are left alone); quantize == 0: (float)y.
 *   Every sample and tap read is bounded by the tables' own ranges; a plan with up or down outside [1, 1024] or a filter outside
 *   [0, n_taps) reads nothing and writes zeros.  1 <= K <= 2^20, n_taps >= 1; null pointers and anything else return -22 before any
 *   launch.  One launch, no workspace, no atomics: bitwise repeatable.  out has sum of N_k floats. */
int mtl_resample(void* stream, const float* wav, const long* offsets, const long* out_offsets, const long* plan, const double* taps,
                 long n_taps, int K, int quantize, float* out);
/* Log-mel filterbank front-end for a sampled batch of K utterances in two launches (csrc/mtl_fbank.hip; LogFBankDataset.parse_audio,
 * utils/data_loader.py:145-155 per utterance: logfbank(sig, rate, nfilt = 80) of python_speech_features with its defaults; that library
 * is not reproduced from its source: the behaviour is DEFINED in DESIGN.md section 15, parity unpinned).  wav / offsets as in
 * mtl_spect_batch (utterance k: L_k >= 1 samples of pcm16 / 32768).  Per utterance: s = 32768 x, p[0] = s[0], p[i] = s[i] - 0.97 s[i-1];
 * T_k = 1 for L_k <= fl, else 1 + ceil((L_k - fl) / fs); frame t = p[t fs .. t fs + fl), zeros past L_k, rectangular window;
 * P[t][f] = |DFT_nfft(frame t)[f]|^2 / nfft for f = 0 .. nfft / 2; E[j][t] = sum_f w[j][f] P[t][f]; v = ln E, or ln(2^-52) where E == 0.
 *   basis: fl x ldb floats, row n = cos(2 pi f n / nfft) for f = 0 .. nfft / 2, then -sin(...) for the same bins (ldb >= nfft + 2)
 *   band: nfilt x 3 ints (first bin, count, offset into band_w): w[j][first + i] = band_w[offset + i], i < count, every other weight 0;
 *     band_w has n_w floats.  A band whose range leaves [0, nfft / 2] or [0, n_w) is read as empty.
 *   out: (K, nfilt, Tmax) fp32, out[k][j][t] = v for t < min(T_k, Tmax) and 0 behind; normalize != 0: (v - mean_k) / std_k with the
 *     statistics in fp64 over ALL nfilt T_k values of utterance k (unbiased std), also when Tmax < T_k.  The std is used as it comes, as in
 *     mtl_spect_batch: an utterance without variance is divided by zero.
 * The frames are formed inside the kernel from an LDS-staged span (no frame matrix and no power spectrum in memory), the DFT runs on
 * v_mfma_f32_16x16x4_f32, the statistics are fp64 partials combined in a fixed order: bitwise repeatable, no atomics, and utterance k's
 * rows depend on utterance k alone.  The grid does not depend on the lengths.  A workgroup takes mtl_fbank_tile_frames() consecutive
 * frames at a time and mtl_fbank_slots() workgroups share an utterance.  workspace: mtl_fbank_batch_workspace(K) bytes, 8-byte aligned.
 * K < 1, fl < 1, fl > nfft, fs < 1, nfilt < 1, Tmax < 1, nfft odd or outside [2, 512], ldb < nfft + 2, n_w < 1, a null pointer or a short
 * workspace return -22 before any launch. */
long mtl_fbank_batch_workspace(int K);
int mtl_fbank_tile_frames(void);
int mtl_fbank_slots(void);
int mtl_fbank_batch(void* stream, const float* wav, const long* offsets, int K, int fl, int fs, int nfft, const float* basis, int ldb,
                    int nfilt, const int* band, const float* band_w, int n_w, float* out, int Tmax, int normalize, void* workspace,
                    long workspace_bytes);
/* SpecAugment (Park et al., 2019) on the finished batch, BEHIND either feature launch (csrc/mtl_specaug.hip; frontend.SpecAugment and
 * DESIGN.md section 23 hold the definition, tests/specaug_util.py restates it in numpy / fp64).  x: the (K, F, Tmax) fp32 batch, changed
 * in place; table: K rows of 3 + 2 freq_masks + 2 time_masks ints on the device: tau, c, w, then (f0, f) per frequency mask, then (t0, t)
 * per time mask.  Per utterance k, over columns [0, tau) only (columns >= tau are never written), in this order:
 *   warp   when w != c: out[j] = x[i0] for a == 0, else fmaf(a, x[i0 + 1] - x[i0], x[i0]) in fp32, the same map for every row:
 *          j < w: num = (2 j + 1) c - w, den = 2 w, base = 0; j >= w: num = (2 (j - w) + 1) (tau - c) - (tau - w), den = 2 (tau - w),
 *          base = c; q = floor(num / den), r = num - q den, i0 = base + q, a = (float)((double)r / (double)den); i0 < 0: i0 = 0, a = 0;
 *          i0 >= tau - 1: i0 = tau - 1, a = 0.  w == c: the row is neither read nor written by this step.
 *   freq   rows [f0, f0 + f) become +0.0f over [0, tau)
 *   time   frames [t0, t0 + t) become +0.0f in every row
 * One launch, one workgroup per (utterance, row): a warped row is read once into LDS and written back warped and masked; a row that is not
 * warped is never read, only its masked spans are stored.  No workspace, no atomics: bitwise repeatable.  The table lives on the device,
 * so the kernel cannot refuse it: tau is cut to [0, Tmax], every span to the plane, and a warp with w outside [1, tau - 1] or c outside
 * [0, tau] is left out -- a wrong table cannot read or write out of bounds.  1 <= K, 1 <= F, K F < 2^31, 1 <= Tmax <= 16384 (a row in
 * 64 KB of LDS), 0 <= freq_masks, time_masks <= 8; null pointers and anything else return -22 before any launch. */
#define MTL_SPECAUG_MAX_MASKS 8
#define MTL_SPECAUG_MAX_FRAMES 16384
int mtl_spec_augment(void* stream, float* x, int K, int F, int Tmax, const int* table, int freq_masks, int time_masks);

/* ---- accent discriminator on the encoder output (joint_train.py --multitask / --adversarial) ------------------------------
 * modules/discriminator.py, trainer/asr/joint_trainer.py:29-37, utils/metrics.py:164-199 (csrc/mtl_disc.hip):
 *   pooled[b][:] = sum_t enc[b][t][:]                      all T rows: the encoder leaves the rows beyond an utterance's length at zero
 *   logits[b][c] = pooled[b] . W[c] + bias[c]              Discriminator.linear, W (C, d), bias (C)
 *   losses[0]    = mean_b ( logsumexp(logits[b]) - logits[b][accent_id] )          F.cross_entropy(logits, [accent_id] * B)
 *   losses[1]    = mean_{b,c} ( logits[b][c] - 1/C )^2                              F.mse_loss(logits, 1/C), mode 1 only
 * mode 0 = multi-task (CE only), 1 = adversarial (CE and MSE).
 * mtl_disc_fwd: enc is (B T, d), rows in (b, t) order.  The time sum is a two-stage reduction in a fixed order, no atomics: stage 1,
 *   workgroups over (b, chunk of MTL_DISC_CHUNK rows), writes per-chunk column sums into `workspace` with 16-byte loads along d;
 *   stage 2 adds an utterance's partials in chunk order and forms its logits; a third launch forms the losses.  pooled (B, d) and
 *   logits (B, C) are outputs, kept by the caller for the backward.
 * mtl_disc_bwd, for the loss  a losses[0] + b losses[1]  (b counts in mode 1 only):
 *   dlogit[b][c]  = a (softmax(logits[b])[c] - [c == accent_id]) / B + b 2 (logits[b][c] - 1/C) / (B C)
 *   dW[c][:]     += sum_b dlogit[b][c] pooled[b][:] ,  dbias[c] += sum_b dlogit[b][c]                    (both in batch order)
 *   denc[b][t][:] += sum_c dlogit[b][c] W[c][:]   for every t < T     (one read-modify-write of denc, 16 bytes per lane)
 * mtl_disc_loss_fwd / mtl_disc_loss_bwd: the loss half alone on given logits (B, C) -- the launches the two calls above end / begin
 *   with; the backward WRITES dlogits (calculate_adversarial / calculate_multi_task on arbitrary logits).
 * mtl_disc_bwd_dlogits: the three accumulations of mtl_disc_bwd for a GIVEN dlogit (B, C) (the gradient autograd hands to the logits).
 * Limits: 1 <= C <= 64, 0 <= accent_id < C, d % 4 == 0, 1 <= B <= 65535, T >= 1, enc / denc / W / workspace 16-byte aligned,
 *   ws_bytes >= mtl_disc_workspace(B, T, d); anything else returns -22 before any launch. */
#ifndef MTL_DISC_CHUNK
#define MTL_DISC_CHUNK 16   /* rows of one utterance per stage-1 workgroup */
#endif
long mtl_disc_workspace(int B, int T, int d);
int mtl_disc_fwd(void* stream, const float* enc, int B, int T, int d, const float* W, const float* bias, int C, int accent_id, int mode,
                 float* pooled, float* logits, float* losses, float* workspace, long ws_bytes);
int mtl_disc_bwd(void* stream, const float* pooled, const float* logits, const float* W, int accent_id, int B, int T, int d, int C, int mode,
                 float a, float b, float* dW, float* dbias, float* denc);
int mtl_disc_bwd_dlogits(void* stream, const float* pooled, const float* dlogits, const float* W, int B, int T, int d, int C, float* dW,
                         float* dbias, float* denc);
int mtl_disc_loss_fwd(void* stream, const float* logits, int B, int C, int accent_id, int mode, float* losses);
int mtl_disc_loss_bwd(void* stream, const float* logits, int B, int C, int accent_id, int mode, float a, float b, float* dlogits);

/* ---- LSTM cell, one time step (lm/model/rnn_model.py:20 nn.LSTM; lm/main_meta_transfer.py:277-411) ----------
 * gx = x_t . W_ih^T + b_ih and gh = h_{t-1} . W_hh^T + b_hh come from mtl_gemm_f32_ex (B x 4H each, torch gate order i|f|g|o).
 * forward: acts = activated gates (saved), c = f*c_prev + i*g, h = o*tanh(c); h_drop (nullable) = h [* mask * mscale]: the
 * copy that feeds the next layer (nn.LSTM's inter-layer dropout) / the decoder (self.drop).
 * backward: dh = dh_up [* mask * mscale] + dh_rec (both nullable), dc = dc_next (nullable) + dh*o*(1-tanh(c)^2);
 * dgates = pre-activation gradients (B x 4H), dc_prev = dc*f. */
int mtl_lstm_cell_fwd(void* stream, const float* gx, const float* gh, const float* c_prev, float* acts, float* c, float* h,
                      float* h_drop, const unsigned char* mask, float mscale, int B, int H);
int mtl_lstm_cell_bwd(void* stream, const float* dh_up, const unsigned char* mask, float mscale, const float* dh_rec,
                      const float* dc_next, const float* acts, const float* c, const float* c_prev, float* dgates, float* dc_prev,
                      int B, int H);
/* Persistent LSTM layer (csrc/mtl_lstm.hip; lm/model/rnn_model.py:20 nn.LSTM over a bptt window): ALL T time steps of one layer in one
 * launch per direction.  Workgroup w owns hidden units [8 w, 8 w + 8) for the whole sequence (its 32 gate rows of W_hh stay in
 * registers), one grid-wide hand-off per step (write-through payload + arrival counter, bounded spins; the grid is H / 8 <= 64
 * workgroups).  The backward splits dh_rec = dG_{t+1} W_hh by rows: every workgroup publishes the partial of its own 32 columns of dG
 * and sums the partials of its 8 units in a fixed order (two partial buffers in the workspace).
 *   forward : gx (T B, 4H) = x W_ih^T + b_ih of all steps (one product), hall / call (T + 1, B, H) with slot 0 = the incoming state;
 *             writes hall[1..T], call[1..T], acts (T B, 4H) [i|f|g|o after the nonlinearities], xout (T B, H) = h (dropout applied when
 *             mask != NULL: u8 keep flags, scale mscale) -- exactly what T calls of the recurrent product + mtl_lstm_cell_fwd produce.
 *   backward: dx_up (T B, H) gradient of xout (may be NULL), writes dG (T B, 4H) = gradient of the gate pre-activations of every step
 *             (truncated BPTT: no gradient into the incoming state) -- what T calls of mtl_lstm_cell_bwd + the dh_rec product produce.
 * workspace: mtl_lstm_layer_workspace() bytes of device memory, 256-byte aligned (4 KB header: arrival counter, per-workgroup step flags and the
 * error word -- u32 [1] != 0 after a timed-out wait; sticky: launches do not clear it, the caller zeroes the workspace once and checks the
 * word whenever it synchronises anyway -- followed by the backward's partial buffers).
 * mtl_lstm_layer_supported: 1 <= B <= 32 and H in {128, 256, 384, 512}; other shapes take the per-step calls. */
int mtl_lstm_layer_supported(int B, int H);
long mtl_lstm_layer_workspace(void);
int mtl_lstm_layer_fwd(void* stream, const float* gx, const float* w_hh, const float* b_hh, float* hall, float* call, float* acts,
                       float* xout, const unsigned char* mask, float mscale, int T, int B, int H, void* workspace);
int mtl_lstm_layer_bwd(void* stream, const float* dx_up, const unsigned char* mask, float mscale, const float* w_hh, const float* acts,
                       const float* call, float* dG, int T, int B, int H, void* workspace);

/* The whole layer stack as ONE wavefront launch per direction (csrc/mtl_lstm.hip; lm/model/rnn_model.py:20 nn.LSTM(ninp, nhid, nlayers,
 * dropout=...)): layer l runs one step behind layer l - 1 instead of after it.  `layers` is a HOST struct of device pointers, one
 * entry per layer (read during the call; not recordable in a command list): gx[0] holds layer 0's input contributions
 * x W_ih0^T + b_ih0 over all T steps (w_ih[0] / b_ih[0] are not used), gx[l >= 1] is T B x 4H scratch the call fills; layers >= 1
 * must have input width H; hall/call/acts/xout/mask/dG as in the single-layer calls (mask[l]: the dropout on layer l's output, or
 * NULL).
 *   forward : fills hall, call, acts, xout of every layer.
 *   backward: fills dG of every layer from dx_up (gradient w.r.t. the top layer's dropped output); scratch = mtl_lstm_stack_scratch()
 *             bytes (the per-step partial sums handed from a layer to the one below).
 * Results equal the per-layer calls up to the summation order of the input contribution (formed per step instead of by one product).
 * mtl_lstm_stack_supported: the single-layer limits, NL <= 4 and (2 NL - 1) * H / 8 <= 224 workgroups (all resident). */
#define MTL_LSTM_MAX_LAYERS 4
typedef struct mtl_lstm_stack {
    const float *w_ih[MTL_LSTM_MAX_LAYERS], *b_ih[MTL_LSTM_MAX_LAYERS], *w_hh[MTL_LSTM_MAX_LAYERS], *b_hh[MTL_LSTM_MAX_LAYERS];
    float *gx[MTL_LSTM_MAX_LAYERS], *hall[MTL_LSTM_MAX_LAYERS], *call[MTL_LSTM_MAX_LAYERS], *acts[MTL_LSTM_MAX_LAYERS], *xout[MTL_LSTM_MAX_LAYERS], *dG[MTL_LSTM_MAX_LAYERS];
    const unsigned char* mask[MTL_LSTM_MAX_LAYERS];
} mtl_lstm_stack;
int mtl_lstm_stack_supported(int B, int H, int NL);
long mtl_lstm_stack_scratch(int T, int B, int H, int NL);
int mtl_lstm_stack_fwd(void* stream, const mtl_lstm_stack* layers, float mscale, int T, int B, int H, int NL, void* workspace);
int mtl_lstm_stack_bwd(void* stream, const mtl_lstm_stack* layers, const float* dx_up, float mscale, float* scratch, int T, int B, int H,
                       int NL, void* workspace);

/* ---- GRU (csrc/mtl_gru.hip; lm/model/rnn_model.py:21 nn.GRU, `--model GRU`) -------------------------------------------------------
 * torch gate order r | z | n.  gx = x_t . W_ih^T + b_ih and gh = h_{t-1} . W_hh^T + b_hh come from mtl_gemm_f32_ex (B x 3H each):
 *   r = sigmoid(gx_r + gh_r), z = sigmoid(gx_z + gh_z), q = gh_n, n = tanh(gx_n + r q), h = (1 - z) n + z h_prev.
 * One time step, element-wise (any B H):
 *   forward : acts (B x 4H) = r | z | n | q (saved), h, h_drop (nullable) = h [* mask * mscale] as in mtl_lstm_cell_fwd.
 *   backward: dh = dh_up [* mask * mscale] + dh_rec + carry_in (all three nullable; the last step has neither dh_rec nor carry_in);
 *             dn = dh (1 - z), dz = dh (h_prev - n), da_n = dn (1 - n^2), dq = da_n r, da_r = da_n q r (1 - r), da_z = dz z (1 - z);
 *             dgx (B x 3H) = da_r | da_z | da_n  (-> W_ih, b_ih, the input gradient), dgh (B x 3H) = da_r | da_z | dq  (-> W_hh, b_hh,
 *             dh_rec of the step before), carry_out (B x H) = dh z  (straight to the same unit of the step before; may alias carry_in). */
int mtl_gru_cell_fwd(void* stream, const float* gx, const float* gh, const float* h_prev, float* acts, float* h, float* h_drop,
                     const unsigned char* mask, float mscale, int B, int H);
int mtl_gru_cell_bwd(void* stream, const float* dh_up, const unsigned char* mask, float mscale, const float* dh_rec,
                     const float* carry_in, const float* acts, const float* h_prev, float* dgx, float* dgh, float* carry_out, int B,
                     int H);
/* Persistent GRU layer: ALL T time steps of one layer in one launch per direction, with the ownership, the hand-off and the workspace
 * of the persistent LSTM layer (above): workgroup w owns hidden units [8 w, 8 w + 8), its 24 gate rows of W_hh stay in registers, one
 * grid-wide hand-off per step, bounded spins, sticky error word u32 [1] of the workspace.
 *   forward : gx (T B, 3H) of all steps, hall (T + 1, B, H) with slot 0 = the incoming state; writes hall[1..T], acts (T B, 4H) = r|z|n|q
 *             and xout (T B, H, nullable) -- what T calls of the recurrent product + mtl_gru_cell_fwd produce.
 *   backward: dx_up (T B, H) gradient of xout (may be NULL); writes dgx and dgh (T B, 3H each) of every step (truncated BPTT: no gradient
 *             into the incoming state) -- what T calls of mtl_gru_cell_bwd + the dh_rec product produce.
 * workspace: mtl_lstm_layer_workspace() bytes, the LSTM launches' own (launches on one stream share it).
 * mtl_gru_layer_supported: the shapes of mtl_lstm_layer_supported. */
int mtl_gru_layer_supported(int B, int H);
int mtl_gru_layer_fwd(void* stream, const float* gx, const float* w_hh, const float* b_hh, float* hall, float* acts, float* xout,
                      const unsigned char* mask, float mscale, int T, int B, int H, void* workspace);
int mtl_gru_layer_bwd(void* stream, const float* dx_up, const unsigned char* mask, float mscale, const float* w_hh, const float* acts,
                      const float* hall, float* dgx, float* dgh, int T, int B, int H, void* workspace);

/* ---- LM sequence NLL (csrc/mtl_lstm.hip; utils/lm.py:42-155 LM.evaluate: LM rescoring of finished beam hypotheses) ------------
 * x (R x H, leading dimension ldx): the top LSTM layer's outputs, rows ordered (t, b) with R = T B; W (V x H), bias (V, nullable):
 * the vocabulary projection (decoder.weight / decoder.bias); target (R) int64, < 0 = skipped row.
 * row_nll[r] = logsumexp_v(x_r W_v^T + b_v) - (x_r W_target^T + b_target)  (0 for skipped rows, NaN for a target >= V);
 * seq_nll[b] (nullable) = sum over t of row_nll[t B + b], in t order.  The R x V logits are never written: one pass over (row tile x
 * vocabulary split) with exact-fp32 MFMA keeps (max, sum-exp, target logit) per split, a second merges the splits in a fixed order.
 * No atomics: bitwise reproducible.  ws: mtl_lm_nll_workspace(R, V) bytes of device memory (4-byte aligned). */
long mtl_lm_nll_workspace(int R, int V);
int mtl_lm_nll_fwd(void* stream, const float* x, int ldx, const float* W, const float* bias, const long* target, int R, int H, int V,
                   int B, float* row_nll, float* seq_nll, void* ws, long ws_bytes);

/* ---- LM evaluation (csrc/mtl_lstm.hip; lm/test.py:189-368 evaluate / evaluate_test): what follows mtl_lm_nll_fwd's row_nll ----------
 * mtl_lm_switch_keys: the language-transition class of every (input word, target word) pair.  ids, target (R) int64; lang (V) bytes,
 * 1 = a Chinese word, 0 = any other.  key[r] = -1 when target[r] < 0, when either id is outside [0, V) or when either id equals eos_id
 * (the reference skips pairs that touch <eos>); else (lang[ids[r]] ? 0 : 2) + (lang[target[r]] ? 0 : 1): 0 = zh->zh, 1 = zh->en,
 * 2 = en->zh, 3 = en->en.
 * mtl_nll_key_sum: sum[k] = sum of row_nll[r] over the rows with key k, accumulated in fp64, count[k] = the number of those rows.  With
 * key == NULL the key of row r is r / seg_rows (equal segments, the last one ragged: the window sums of an evaluation).  Rows whose key
 * is outside [0, nkey) are skipped; every sum[k] and count[k] is written (0 for a key without rows).  No atomics: each key's rows are
 * added by one owner thread per block of 256 rows in row order and the blocks are merged in block order, so the results are
 * bit-identical from run to run.  -22 for nkey > MTL_NLL_MAX_KEYS, R < 1, nkey < 1, seg_rows < 1 with a null key, a null operand or a
 * workspace below mtl_nll_key_sum_workspace(R, nkey) bytes (8-byte aligned device memory). */
#define MTL_NLL_MAX_KEYS 4096
int mtl_lm_switch_keys(void* stream, const long* ids, const long* target, const unsigned char* lang, long eos_id, int R, int V, int* key);
long mtl_nll_key_sum_workspace(int R, int nkey);
int mtl_nll_key_sum(void* stream, const float* row_nll, const int* key, int seg_rows, int R, int nkey, double* sum, int* count, void* ws,
                    long ws_bytes);

/* ---- LM epoch training (csrc/mtl_lstm.hip; lm/main.py:256-277): mtl_embed_bwd's occurrence chains of every window of a stream ---------
 * ids (S, B) int64, batchified.  Windows start at i = 0, bptt, ... < S - 1; window i has T = min(bptt, S - 1 - i) steps and R = T B rows
 * in (t, b) order at flat offset i B.  For row r of a window: first[i B + r] = 1 iff no earlier row of the SAME window holds the same id,
 * else 0; next[i B + r] = the window-relative index of the next row of the same window with the same id, or -1.  Chains never cross a
 * window; first and next hold (S - 1) B ints each.  One launch, a workgroup per window.  -22 before any launch for a window of more than
 * mtl_lm_window_chains_max_rows() rows, S < 2, B < 1, bptt < 1 or a null pointer. */
int mtl_lm_window_chains_max_rows(void);
int mtl_lm_window_chains(void* stream, const long* ids, long S, int B, int bptt, int* first, int* next);

/* ---- device-resident beam search (csrc/mtl_beam.hip; modules/decoder.py:187-291 Decoder.beam_search) --------------------------
 * A chunk of U utterances is searched at once: W hypothesis rows per utterance, row u W + r of every (U W, ...) operand.
 * Limits (anything beyond is refused with -22): 1 <= W <= MTL_BEAM_MAX_W, W <= V <= MTL_BEAM_MAX_V, 1 <= S <= MTL_BEAM_MAX_S
 * positions, U <= MTL_BEAM_MAX_U, at most MTL_BEAM_MAX_CACHES caches per gather.
 *
 * mtl_beam_rank: what modules/decoder.py:215-280 does between two decoder steps, for position i of all U utterances in ONE launch
 * (a workgroup per utterance).  logits (U W, V) and lse (U W) = log-sum-exp of each row (mtl_ce_argmax_fwd's `lse`).  Selection rule:
 *   - live row r (row order) offers the W largest  local = logit - lse  (fp32) of its row, largest first, equal values resolving to the
 *     LOWER vocabulary id; candidate score = fp32(score_r + local);
 *   - the W best of the n W candidates survive, equal scores resolving to the EARLIER (row, rank) pair (a stable descending sort of the
 *     candidates in (row, rank) order, cut at W -- equal to the reference's cumulative sorted(...)[:W]); survivors keep that order;
 *   - at i == T4 - 1 every survivor ends with a forced EOS appended behind its token;
 *   - survivors ending in EOS are appended to the utterance's ended list (survivor order), the others become live rows 0..n'-1.
 * state: mtl_beam_state_words(U, W, S) int32 words (fp32 values as their bit patterns):
 *   hdr   [U][4]        live rows n | done flag | ended entries | reserved      (start of a search: 1, 0, 0, 0)
 *   score [U][W]   f32  score of live row r                                     (start: score[u][0] = 0)
 *   bp    [U][S][W]     bp[u][i][r'] = live row BEFORE position i that live row r' AFTER position i continues
 *   tk    [U][S][W]     tk[u][i][r'] = the token appended at position i
 *   ended [U][S W][5]   position | score (f32) | live row before that position | token | 1 = EOS forced behind the token, 0 = token is the EOS
 * so the sequence of live row r before position i is  seq(i, r) = seq(i - 1, bp[i-1][r]) + [tk[i-1][r]],  seq(0, 0) = [start token],
 * and an ended entry is  seq(position, row) + [token] (+ [EOS] when forced).
 * Outputs for position i + 1: tok (U W) int64 = the live rows' tokens (rows n'.. are fed eos_id), parent (U W) int32 = the GLOBAL row
 * u W + bp whose caches row u W + r' continues (rows n'..: the utterance's row 0).  An utterance is done (flag set) when no live row is
 * left; the kernel returns at once for a done utterance and leaves its state, tok and parent untouched (the step that finishes it
 * writes the identity into its parent rows).
 *
 * mtl_beam_gather: caches[c][r, :t] <- caches[c][parent[r], :t] for c < ncache, with `parent` read from device memory.  caches_dev:
 * DEVICE table of ncache pointers to (rows, S', width) fp32 caches, 16-byte aligned, row_stride floats between two rows (>= t width;
 * width and row_stride multiples of 4).  Never permutes in place: the moved rows go to tmp (>= ncache rows t width floats, 16-byte
 * aligned) and are copied back by a second launch; rows with parent[r] == r are not touched. */
#define MTL_BEAM_MAX_W 8
#define MTL_BEAM_MAX_V (1 << 20)
#define MTL_BEAM_MAX_S 4096
#define MTL_BEAM_MAX_U 64
#define MTL_BEAM_MAX_CACHES 64
long mtl_beam_state_words(int U, int W, int S); /* -22 beyond the limits */
int mtl_beam_rank(void* stream, const float* logits, const float* lse, int* state, long* tok, int* parent, int i, int T4, int U, int W,
                  int V, int S, int eos_id);
int mtl_beam_gather(void* stream, float* const* caches_dev, int ncache, const int* parent, float* tmp, long tmp_floats, int rows, int t,
                    int width, long row_stride);

/* ---- CTC loss (--loss ctc): utils/metrics.py:127-148 = F.ctc_loss(log_softmax(pred), gold, sizes, trg_lengths, 'mean') ------------
 * U utterances of T rows each: logits (U T, ld) fp32, gold one row of ldg int64 per utterance of which the first tgt_len[u] entries
 * are the labels, in_len / tgt_len (U) int32 ON THE DEVICE.  The kernels clamp in_len to [0, T] and tgt_len to [0, min(Lmax, ldg)];
 * an utterance with a label outside [0, V) is infeasible.  The forward forms each row's log-sum-exp itself, as an fp32 pair hi + lo
 * (mtl_ce_argmax_fwd's single-fp32 `lse` would put its rounding, 1e-6 at |logit| ~ 30, into every log-probability).
 *   nll[u]      = -log p(labels_u | rows 0..in_len[u]-1), +inf when no alignment exists (also in_len = 0 with tgt_len > 0; 0 when both
 *                 are 0), exactly reduction='none' with zero_infinity=False
 *   loss_out[g] = sum over the per_group utterances of group g of nll_u / max(tgt_len_u, 1), / per_group   (U % per_group == 0; one
 *                 loss per task, per_group = U is reduction='mean')
 *   dlogits     = gscale * (gscale_dev ? gscale_dev[g] : 1) / (per_group max(tgt_len_u, 1)) * (softmax - label posterior) on the rows
 *                 t < in_len[u] of a feasible utterance; exactly 0 on the other rows, on EVERY row of an infeasible utterance (torch's
 *                 zero_infinity=True gradient; with False it writes NaN there) and in the columns V..ldd-1.  Every element of the
 *                 (U T, ldd) rows is written.  Bitwise reproducible from run to run.
 * ws (8-byte aligned): what the forward leaves for the backward -- the row statistics (U T) x 2 fp32 and the log-alpha lattice
 * (U, T, 2 Lmax + 1) fp32 -- mtl_ctc_workspace bytes (-22 for U, T or Lmax outside 1.., Lmax > MTL_CTC_MAX_L).  Stream-ordered, no
 * allocation, recordable. */
#define MTL_CTC_MAX_L 1400
long mtl_ctc_workspace(int U, int T, int Lmax);
int mtl_ctc_fwd(void* stream, const float* logits, const long* gold, const int* in_len, const int* tgt_len, int U, int T, int V, int ld,
                int ldg, int Lmax, int blank, int per_group, float* ws, long ws_bytes, float* nll, float* loss_out);
int mtl_ctc_bwd(void* stream, const float* logits, const long* gold, const int* in_len, const int* tgt_len, int U, int T, int V, int ld,
                int ldg, int Lmax, int blank, int per_group, const float* ws, long ws_bytes, const float* nll, float gscale,
                const float* gscale_dev, float* dlogits, int ldd);

/* ---- raw byte helpers on a stream (so that a whole task body consists of library calls only and can be replayed) ---- */
int mtl_memset_zero(void* stream, void* dst, long bytes);
int mtl_memcpy_d2d(void* stream, void* dst, const void* src, long bytes);
/* hipEventRecord / hipStreamWaitEvent on caller-owned handles (fork / join of the parameter-gradient side stream) */
int mtl_event_record(void* event, void* stream);
int mtl_stream_wait_event(void* stream, void* event);

/* ---- command lists: ONE call from the host language replays a recorded sequence of the calls above ------------------------
 * The per-task body of the meta step (trainer/asr/transient_trainer.py:178-237: train pass, inner SGD, validation pass,
 * copy_grad accumulation) is ~700 library calls whose arguments -- device pointers into the caller's static buffers, shapes,
 * scalars, stream and event handles -- do not change from task to task: everything batch-dependent lives in device buffers the
 * host refreshes before the replay.  The host layer records the calls of one eager run (`mtl_cmd` entries: opcode = position of
 * the function in this header's declaration order, see mtl_cmdlist_opcode; arguments in declaration order, one 8-byte slot
 * each: pointers / integers as-is, floats as double) and afterwards issues mtl_cmdlist_run, which performs exactly those calls
 * in order from C.  Returns 0, or the first failing call's code with *failed_index = its position (nullable). */
typedef struct mtl_cmd {
    int op;
    int nargs;
    union {
        void* p;
        long l;
        double d;
    } a[48];
} mtl_cmd;
int mtl_cmdlist_opcode(const char* function_name);     /* -1 if the function cannot be recorded */
int mtl_cmdlist_run(const mtl_cmd* cmds, int n, int* failed_index);
/* diagnostics: the same replay, and host_us[i] = HOST time (microseconds) the i-th call took to return (a launch that blocks in
 * the runtime -- full queue, exhausted kernel-argument pool, a signal still in use -- shows up here, not in any device profile) */
int mtl_cmdlist_run_timed(const mtl_cmd* cmds, int n, int* failed_index, float* host_us);

/* ---- host helper: Levenshtein distance on code points (utils/metrics.py:38-44 uses python-Levenshtein) ---- */
int mtl_levenshtein_u32(const unsigned int* a_host, int na, const unsigned int* b_host, int nb);

#ifdef __cplusplus
}
#endif
#endif /* MTL_HIP_H */
