// Device-resident beam search (modules/decoder.py:187-291): hypothesis ranking between two decoder steps and the K/V-cache gather
// that follows it.  Both are latency-bound (a position of the search is a chain of ~50 small launches), so each is as few launches as
// its hazards allow: ONE for the ranking of all utterances of a chunk, two for the gather (out to a second buffer, copy back).
//
// Selection rule of mtl_beam_rank (what the host-ranked PassEngine.beam_decode and the reference compute):
//   candidates   live row r (in row order) contributes the W largest  local = logit - lse  (fp32) of its V entries, largest first;
//                equal values resolve to the LOWER vocabulary id.  Candidate score = fp32(score_r + local).
//   survivors    the W best of the n W candidates by score; equal scores resolve to the EARLIER (row, rank) pair -- a stable
//                descending sort of the candidates in (row, rank) order, cut at W.  (The reference sorts cumulatively inside its
//                hypothesis loop and cuts at W after every row: a candidate dropped there already had W candidates ahead of it, so the
//                result is this stable global top-W.)  Survivors are kept in sorted order.
//   forced EOS   at position T4 - 1 every survivor ends, an EOS appended behind its token (even when that token is EOS itself).
//   split        survivors ending in EOS join the ended list in survivor order; the others become live rows 0..n'-1 in survivor order.
#include <climits>

#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

__device__ __forceinline__ bool cand_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// one workgroup (4 waves) per utterance
__global__ __launch_bounds__(256) void beam_rank_kernel(const float* __restrict__ logits, const float* __restrict__ lse, int* __restrict__ state,
                                                        long* __restrict__ tok, int* __restrict__ parent, int i, int T4, int U, int W, int V,
                                                        int S, int eos) {
    const int u = blockIdx.x;
    int* hdr = state + 4 * u;
    if (hdr[1]) return;                                   // finished utterance: state untouched (uniform for the workgroup)
    const int n = min(max(hdr[0], 0), W);
    float* score = reinterpret_cast<float*>(state + 4 * (long)U) + (long)u * W;
    int* bp = state + 4 * (long)U + (long)U * W + ((long)u * S + i) * W;
    int* tk = bp + (long)U * S * W;
    int* ended = state + 4 * (long)U + (long)U * W + 2 * (long)U * S * W + (long)u * S * W * 5;

    __shared__ float c_score[MTL_BEAM_MAX_W * MTL_BEAM_MAX_W];
    __shared__ int c_tok[MTL_BEAM_MAX_W * MTL_BEAM_MAX_W];
    __shared__ float s_score[MTL_BEAM_MAX_W];
    __shared__ int s_tok[MTL_BEAM_MAX_W], s_par[MTL_BEAM_MAX_W];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- candidates: a wave per live row; W passes over the row, pass j takes the best entry that comes AFTER pick j - 1 in the order
    // (value descending, id ascending).  A row is 15 KB from L2 and a pass is V / 64 loads per lane: the passes cost less than a launch.
    for (int r = wave; r < n; r += 4) {
        const float* x = logits + ((long)u * W + r) * V;
        const float l = lse[u * W + r], sc = score[r];
        float pv = 0.f;
        int pid = -1;
        for (int j = 0; j < W; ++j) {
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int v = lane; v < V; v += 64) {
                const float loc = x[v] - l;
                const bool after = j == 0 || cand_better(pv, pid, loc, v);
                if (after && cand_better(loc, v, bv, bi)) bv = loc, bi = v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (cand_better(ov, oi, bv, bi)) bv = ov, bi = oi;
            }
            if (lane == 0) {
                c_score[r * W + j] = sc + bv;
                c_tok[r * W + j] = bi == INT_MAX ? eos : bi;          // (no orderable entry left -- NaN logits: keep the id in range)
            }
            pv = bv, pid = bi;
        }
    }
    __syncthreads();
    // ---- survivors: candidate c's place in the stable descending order = how many candidates come before it
    const int m = n * W;
    if (threadIdx.x < m) {
        const int c = threadIdx.x;
        const float v = c_score[c];
        int place = 0;
        for (int o = 0; o < m; ++o) place += cand_better(c_score[o], o, v, c) ? 1 : 0;
        if (place < W) s_score[place] = v, s_tok[place] = c_tok[c], s_par[place] = c / W;
    }
    __syncthreads();
    // ---- forced EOS, split, outputs (W <= 8 items: one lane)
    if (threadIdx.x == 0) {
        const bool force = i == T4 - 1;
        int ne = hdr[2], nl = 0;
        const int ns = min(m, W);
        for (int k = 0; k < ns; ++k) {
            const int t = s_tok[k], p = s_par[k];
            if (force || t == eos) {
                if (ne < S * W) {
                    int* e = ended + 5 * (long)ne;
                    e[0] = i, e[1] = __float_as_int(s_score[k]), e[2] = p, e[3] = t, e[4] = force ? 1 : 0;
                    ++ne;
                }
            } else {
                score[nl] = s_score[k];
                bp[nl] = p, tk[nl] = t;
                tok[u * W + nl] = t;
                parent[u * W + nl] = u * W + p;
                ++nl;
            }
        }
        for (int r = nl; r < W; ++r) {
            tok[u * W + r] = eos;                                     // padding rows are fed EOS and continue row 0, like the host-ranked search
            parent[u * W + r] = nl ? u * W : u * W + r;               // (an utterance that just finished: nothing moves any more)
        }
        hdr[0] = nl, hdr[2] = ne;
        if (nl == 0) hdr[1] = 1;
    }
}

// dir 0: tmp[c][r][:n] = caches[c][parent[r]][:n]; dir 1: caches[c][r][:n] = tmp[c][r][:n] -- rows that continue themselves are skipped
__global__ __launch_bounds__(256) void beam_gather_kernel(float* const* __restrict__ caches, const int* __restrict__ parent, float* __restrict__ tmp,
                                                          int rows, long row_stride, long n, int dir) {
    const int r = blockIdx.x, c = blockIdx.y;
    const int p = parent[r];
    if (p == r || p < 0 || p >= rows) return;
    float* slot = tmp + ((long)c * rows + r) * n;
    const float4* src = reinterpret_cast<const float4*>(dir ? slot : caches[c] + (long)p * row_stride);
    float4* dst = reinterpret_cast<float4*>(dir ? caches[c] + (long)r * row_stride : slot);
    for (long k = threadIdx.x; k < n / 4; k += 256) dst[k] = src[k];
}

}  // namespace

extern "C" {

long mtl_beam_state_words(int U, int W, int S) {
    if (U <= 0 || W <= 0 || S <= 0 || W > MTL_BEAM_MAX_W || S > MTL_BEAM_MAX_S) return MTL_EINVAL;
    return 4L * U + (long)U * W + 2L * U * S * W + 5L * U * S * W;
}

int mtl_beam_rank(void* stream, const float* logits, const float* lse, int* state, long* tok, int* parent, int i, int T4, int U, int W, int V,
                  int S, int eos_id) {
    if (!logits || !lse || !state || !tok || !parent) return MTL_EINVAL;
    if (U <= 0 || U > MTL_BEAM_MAX_U || W < 1 || W > MTL_BEAM_MAX_W || V < W || V > MTL_BEAM_MAX_V || S < 1 || S > MTL_BEAM_MAX_S) return MTL_EINVAL;
    if (i < 0 || i >= S || T4 < 1 || eos_id < 0 || eos_id >= V) return MTL_EINVAL;
    hipLaunchKernelGGL(beam_rank_kernel, dim3(U), dim3(256), 0, as_stream(stream), logits, lse, state, tok, parent, i, T4, U, W, V, S, eos_id);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_beam_gather(void* stream, float* const* caches_dev, int ncache, const int* parent, float* tmp, long tmp_floats, int rows, int t, int width,
                    long row_stride) {
    if (!caches_dev || !parent || !tmp) return MTL_EINVAL;
    if (ncache < 1 || ncache > MTL_BEAM_MAX_CACHES || rows < 1 || rows > MTL_BEAM_MAX_U * MTL_BEAM_MAX_W || t < 1 || t > MTL_BEAM_MAX_S) return MTL_EINVAL;
    if (width < 4 || (width & 3) || (row_stride & 3) || row_stride < (long)t * width) return MTL_EINVAL;
    if (tmp_floats < (long)ncache * rows * t * width || (reinterpret_cast<uintptr_t>(tmp) & 15)) return MTL_EINVAL;
    const long n = (long)t * width;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(beam_gather_kernel, dim3(rows, ncache), dim3(256), 0, s, caches_dev, parent, tmp, rows, row_stride, n, 0);
    hipLaunchKernelGGL(beam_gather_kernel, dim3(rows, ncache), dim3(256), 0, s, caches_dev, parent, tmp, rows, row_stride, n, 1);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

}  // extern "C"
