// CTC loss and its gradient w.r.t. the logits (log-softmax folded in) for --loss ctc: utils/metrics.py:127-148 of the reference,
// i.e. F.ctc_loss(log_softmax(pred), gold, sizes, trg_lengths, reduction='mean', zero_infinity=False) with blank = PAD.
//
// The CTC "time" axis is the teacher-forced decoder axis: T is short (tens of positions), V is wide (thousands).  Layout:
//   ctc_rowstat_kernel one wave per logits row: the row's log-sum-exp as an unevaluated fp32 PAIR hi + lo.  A single fp32 lse of
//                      magnitude ~30 carries half an ulp (1e-6) of error into every log-probability x - lse, which is all of a
//                      log-probability near 0; (x - hi) - lo keeps it at the rounding of the result, like log_softmax itself.
//   ctc_alpha_kernel   one workgroup per utterance.  Log-space fp32 alpha recursion over t; the extended states s < S = 2 L + 1 are
//                      spread over the 256 lanes with a strided loop (S may exceed the workgroup); the two live alpha rows sit in
//                      LDS, every row also goes to the workspace lattice (U, T, 2 Lmax + 1) for the backward.  Writes nll[u].
//   ctc_loss_kernel    one workgroup per task group: loss[g] = sum_u nll_u / max(L_u, 1) / per_group, summed in a fixed order.
//   ctc_rows_kernel    one wave per logits row: dlogits = gs_u * softmax on rows t < in_len of feasible utterances, 0 elsewhere
//                      (every element of the (U T, ldd) rows is written, the columns V..ldd-1 with zeros).
//   ctc_beta_kernel    one workgroup per feasible utterance.  Beta recursion from t = in_len - 1 down, the two live rows in LDS;
//                      per t the state posteriors exp(alpha + beta - logp + nll) go to LDS and are folded into the columns of
//                      their labels: the blank states (column `blank`) by a fixed-order strided sum + wave/LDS tree, each label by
//                      the FIRST occurrence of that label walking its next-occurrence chain in order (built once in LDS).  Every
//                      column has one writer and one summation order: run-to-run bitwise deterministic, no float atomics.
// No workgroup waits for another one.  Every loop bound is a host-checked scalar or a length clamped to it on the device
// (in_len to [0, T], tgt_len to [0, min(Lmax, ldg)]); a label outside [0, V) makes its utterance infeasible (+inf, zero gradient)
// before anything is indexed with it.  An infeasible utterance has nll = +inf and an all-zero gradient (torch writes NaN there with
// zero_infinity=False; this is torch's zero_infinity=True gradient, identical on feasible utterances).
// Workspace: [row statistics (U T) float2][log-alpha lattice (U, T, 2 Lmax + 1) float].
#include "mtl_common.h"
#include "../../include/mtl_hip.h"

namespace {

constexpr int CTC_THREADS = 256;
constexpr long CTC_LDS_BYTES = 65536;

__device__ __forceinline__ int ctc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// log(exp(a) + exp(b) + exp(c)); -inf when all three are -inf (never (-inf) - (-inf))
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// log-probability of a logit under its row's statistics
__device__ __forceinline__ float ctc_logp(float x, float2 z) { return (x - z.x) - z.y; }

// label of extended state s (lab = the utterance's labels in LDS)
__device__ __forceinline__ int ctc_ext(const int* lab, int s, int blank) { return (s & 1) ? lab[s >> 1] : blank; }

// loads the labels into LDS; returns (through LDS flag) whether all of them are inside [0, V)
__device__ __forceinline__ bool ctc_load_labels(const long* __restrict__ g, int L, int V, int* lab, int* bad) {
    if (threadIdx.x == 0) *bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += CTC_THREADS) {
        const long v = g[i];
        const bool ok = v >= 0 && v < V;
        lab[i] = ok ? (int)v : 0;
        if (!ok) *bad = 1;                       // (benign: every writer stores the same value)
    }
    __syncthreads();
    return *bad == 0;
}

// stat[row] = (hi, lo) with hi + lo = max + log(sum exp(x - max)): hi the fp32 sum, lo its rounding error (two-sum)
__global__ __launch_bounds__(CTC_THREADS) void ctc_rowstat_kernel(const float* __restrict__ logits, int rows, int V, int ld,
                                                                  float2* __restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (CTC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = logits + (long)row * ld;
    float mx = -INFINITY;
    for (int j = lane; j < V; j += 64) mx = fmaxf(mx, x[j]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j < V; j += 64) s += expf(x[j] - mx);
    s = wave_sum(s);
    if (lane == 0) {
        const float ls = logf(s);
        const float hi = mx + ls;
        const float bb = hi - mx;
        const float lo = (mx - (hi - bb)) + (ls - bb);
        stat[row] = make_float2(hi, hi - hi == 0.f ? lo : 0.f);              // (a non-finite row keeps its hi and no NaN correction)
    }
}

__global__ __launch_bounds__(CTC_THREADS) void ctc_alpha_kernel(const float* __restrict__ logits, const float2* __restrict__ stat,
                                                                const long* __restrict__ gold, const int* __restrict__ in_len,
                                                                const int* __restrict__ tgt_len, int T, int V, int ld, int ldg,
                                                                int Lmax, int blank, float* __restrict__ lattice, float* __restrict__ nll) {
    extern __shared__ float smem[];
    const int Smax = 2 * Lmax + 1;
    float* row0 = smem;
    float* row1 = smem + Smax;
    int* lab = reinterpret_cast<int*>(smem + 2 * Smax);
    __shared__ int bad;
    const int u = blockIdx.x, tid = threadIdx.x;
    const int Tin = ctc_clamp(in_len[u], 0, T);
    const int L = ctc_clamp(tgt_len[u], 0, Lmax < ldg ? Lmax : ldg);
    const int S = 2 * L + 1;
    const bool ok = ctc_load_labels(gold + (long)u * ldg, L, V, lab, &bad);
    if (!ok || Tin == 0) {
        if (tid == 0) nll[u] = (ok && L == 0) ? 0.f : INFINITY;
        return;
    }
    const float* x = logits + (long)u * T * ld;
    const float2* z = stat + (long)u * T;
    float* lat = lattice + (long)u * T * Smax;
    float* prev = row0;
    float* cur = row1;
    for (int s = tid; s < S; s += CTC_THREADS) {
        const float a = s < 2 ? ctc_logp(x[ctc_ext(lab, s, blank)], z[0]) : -INFINITY;
        prev[s] = a;
        lat[s] = a;
    }
    __syncthreads();
    // the recursion is a chain of T short steps: the logit of this lane's first state (all of them when S <= 256) is fetched one
    // step ahead, so its latency overlaps the previous step instead of adding to every link of the chain
    const int c0 = tid < S ? ctc_ext(lab, tid, blank) : blank;
    float xn = Tin > 1 ? x[(long)ld + c0] : 0.f;
    for (int t = 1; t < Tin; ++t) {
        const float* xt = x + (long)t * ld;
        const float2 zt = z[t];
        float* lt = lat + (long)t * Smax;
        const float x0 = xn;
        if (t + 1 < Tin) xn = xt[(long)ld + c0];
        for (int s = tid; s < S; s += CTC_THREADS) {
            const int c = ctc_ext(lab, s, blank);
            const float lp = ctc_logp(s == tid ? x0 : xt[c], zt);
            const float a0 = prev[s];
            const float a1 = s >= 1 ? prev[s - 1] : -INFINITY;
            const float a2 = (s >= 2 && ctc_ext(lab, s - 2, blank) != c) ? prev[s - 2] : -INFINITY;
            const float a = ctc_lse3(a0, a1, a2);
            const float v = a == -INFINITY ? -INFINITY : a + lp;
            cur[s] = v;
            lt[s] = v;
        }
        __syncthreads();                                                     // cur complete; prev no longer read
        float* sw = prev;
        prev = cur;
        cur = sw;
    }
    if (tid == 0) {
        const float a = prev[S - 1];
        const float b = S > 1 ? prev[S - 2] : -INFINITY;
        nll[u] = -ctc_lse3(a, b, -INFINITY);
    }
}

// loss[g] = sum over the group's utterances of nll_u / max(L_u, 1), / per_group.  Fixed order: strided partial sums, wave tree, 4 waves.
__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_kernel(const float* __restrict__ nll, const int* __restrict__ tgt_len, int per_group,
                                                               int Lcap, float* __restrict__ loss) {
    __shared__ float part[CTC_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < per_group; i += CTC_THREADS) {
        const int u = g * per_group + i;
        const int L = ctc_clamp(tgt_len[u], 0, Lcap);
        s += nll[u] / (float)(L > 1 ? L : 1);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) loss[g] = ((part[0] + part[1]) + (part[2] + part[3])) / (float)per_group;
}

// per-utterance gradient scale: gscale [* gscale_dev[group]] / (per_group * max(L, 1)); 0 for an infeasible utterance
__device__ __forceinline__ float ctc_gs(int u, const float* nll, const int* tgt_len, int Lcap, int per_group, float gscale,
                                        const float* gscale_dev) {
    if (!(nll[u] < INFINITY)) return 0.f;                                    // +inf (infeasible) and NaN
    if (gscale_dev) gscale *= gscale_dev[u / per_group];
    const int L = ctc_clamp(tgt_len[u], 0, Lcap);
    return gscale / ((float)per_group * (float)(L > 1 ? L : 1));
}

__global__ __launch_bounds__(CTC_THREADS) void ctc_rows_kernel(const float* __restrict__ logits, const float2* __restrict__ stat,
                                                               const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                               const float* __restrict__ nll, int rows, int T, int V, int ld, int Lcap,
                                                               int per_group, float gscale, const float* gscale_dev,
                                                               float* __restrict__ dlogits, int ldd) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (CTC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int u = row / T, t = row - u * T;
    float* d = dlogits + (long)row * ldd;
    const bool live = t < ctc_clamp(in_len[u], 0, T) && nll[u] < INFINITY;
    if (!live) {
        for (int j = lane; j < ldd; j += 64) d[j] = 0.f;
        return;
    }
    const float gs = ctc_gs(u, nll, tgt_len, Lcap, per_group, gscale, gscale_dev);
    const float* x = logits + (long)row * ld;
    const float2 z = stat[row];
    for (int j = lane; j < V; j += 64) d[j] = gs * expf(ctc_logp(x[j], z));
    for (int j = V + lane; j < ldd; j += 64) d[j] = 0.f;
}

__global__ __launch_bounds__(CTC_THREADS) void ctc_beta_kernel(const float* __restrict__ logits, const float2* __restrict__ stat,
                                                               const long* __restrict__ gold, const int* __restrict__ in_len,
                                                               const int* __restrict__ tgt_len, int T, int V, int ld, int ldg,
                                                               int Lmax, int blank, const float* __restrict__ lattice,
                                                               const float* __restrict__ nll, int per_group, float gscale,
                                                               const float* gscale_dev, float* __restrict__ dlogits, int ldd) {
    extern __shared__ float smem[];
    const int Smax = 2 * Lmax + 1;
    float* row0 = smem;
    float* row1 = smem + Smax;
    float* post = smem + 2 * Smax;
    float* slp = smem + 3 * Smax;                // log-probability of each state's label at the current t
    int* lab = reinterpret_cast<int*>(smem + 4 * Smax);
    int* nxt = lab + Lmax;                       // next occurrence of the same label, -1 at the end of a chain
    int* head = nxt + Lmax;                      // 1 = first occurrence of its label
    __shared__ int bad;
    __shared__ float wpart[CTC_THREADS / 64];
    __shared__ float extra;                      // posterior of the labels equal to `blank` (they share the blank states' column)
    const int u = blockIdx.x, tid = threadIdx.x;
    const float nl = nll[u];
    if (!(nl < INFINITY)) return;                // infeasible: ctc_rows_kernel wrote its zeros
    const int Tin = ctc_clamp(in_len[u], 0, T);
    const int Lcap = Lmax < ldg ? Lmax : ldg;
    const int L = ctc_clamp(tgt_len[u], 0, Lcap);
    const int S = 2 * L + 1;
    if (Tin == 0) return;
    if (!ctc_load_labels(gold + (long)u * ldg, L, V, lab, &bad)) return;     // (cannot happen with a finite nll; keeps indexing safe)
    const float gs = ctc_gs(u, nll, tgt_len, Lcap, per_group, gscale, gscale_dev);
    for (int i = tid; i < L; i += CTC_THREADS) head[i] = 1;
    if (tid == 0) extra = 0.f;
    __syncthreads();
    for (int i = tid; i < L; i += CTC_THREADS) {
        const int c = lab[i];
        int j = i + 1;
        while (j < L && lab[j] != c) ++j;
        nxt[i] = j < L ? j : -1;
        if (j < L) head[j] = 0;                  // (j is the successor of exactly one i)
    }
    __syncthreads();
    const float* x = logits + (long)u * T * ld;
    const float2* z = stat + (long)u * T;
    const float* lat = lattice + (long)u * T * Smax;
    float* dl = dlogits + (long)u * T * ldd;
    float* prev = row0;                          // beta of t + 1
    float* cur = row1;
    // as in ctc_alpha_kernel: the logit and the saved alpha of this lane's first state are fetched one step ahead
    const int c0 = tid < S ? ctc_ext(lab, tid, blank) : blank;
    float xn = x[(long)(Tin - 1) * ld + c0];
    float an = tid < S ? lat[(long)(Tin - 1) * Smax + tid] : 0.f;
    for (int t = Tin - 1; t >= 0; --t) {
        const float* xt = x + (long)t * ld;
        const float2 zt = z[t];
        const float* lt = lat + (long)t * Smax;
        const float x0 = xn, al0 = an;
        if (t > 0) {
            xn = xt[c0 - (long)ld];
            if (tid < S) an = lt[tid - (long)Smax];
        }
        for (int s = tid; s < S; s += CTC_THREADS) {
            const int c = ctc_ext(lab, s, blank);
            const float lp = ctc_logp(s == tid ? x0 : xt[c], zt);
            const float al = s == tid ? al0 : lt[s];
            float b;
            if (t == Tin - 1) {
                b = s >= S - 2 ? lp : -INFINITY;
            } else {
                const float b0 = prev[s];
                const float b1 = s + 1 < S ? prev[s + 1] : -INFINITY;
                const float b2 = (s + 2 < S && ctc_ext(lab, s + 2, blank) != c) ? prev[s + 2] : -INFINITY;
                b = ctc_lse3(b0, b1, b2);
                b = b == -INFINITY ? -INFINITY : b + lp;
            }
            cur[s] = b;
            slp[s] = lp;
            // state posterior; an unreachable cell (alpha or beta = -inf) contributes exactly 0
            post[s] = (al == -INFINITY || b == -INFINITY) ? 0.f : expf(al + b + nl - lp);
        }
        __syncthreads();                                                     // post, slp and cur complete
        float* dt = dl + (long)t * ldd;
        for (int i = tid; i < L; i += CTC_THREADS) {
            if (!head[i]) continue;
            float sum = 0.f;
            for (int j = i; j >= 0; j = nxt[j]) sum += post[2 * j + 1];
            const int c = lab[i];
            if (c == blank) extra = sum;
            else dt[c] = gs * (expf(slp[2 * i + 1]) - sum);
        }
        float bs = 0.f;
        for (int k = tid; k <= L; k += CTC_THREADS) bs += post[2 * k];
        bs = wave_sum(bs);
        if ((tid & 63) == 0) wpart[tid >> 6] = bs;
        __syncthreads();                                                     // wpart and extra complete; post no longer read
        if (tid == 0) {
            const float sum = ((wpart[0] + wpart[1]) + (wpart[2] + wpart[3])) + extra;
            dt[blank] = gs * (expf(slp[0]) - sum);
        }
        float* sw = prev;
        prev = cur;
        cur = sw;
    }
}

bool ctc_dims_ok(int U, int T, int V, int Lmax) { return U > 0 && T > 0 && V > 0 && Lmax > 0 && Lmax <= MTL_CTC_MAX_L; }
long ctc_fwd_lds(int Lmax) { return ((long)2 * (2 * Lmax + 1) + Lmax) * 4; }
long ctc_bwd_lds(int Lmax) { return ((long)4 * (2 * Lmax + 1) + 3 * Lmax) * 4; }
bool ctc_ws_ok(const void* ws, long ws_bytes, int U, int T, int Lmax) {
    return ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= mtl_ctc_workspace(U, T, Lmax);
}

}  // namespace

long mtl_ctc_workspace(int U, int T, int Lmax) {
    if (U <= 0 || T <= 0 || Lmax <= 0 || Lmax > MTL_CTC_MAX_L) return MTL_EINVAL;
    return (long)U * T * (2 * (long)Lmax + 1 + 2) * (long)sizeof(float);
}

int mtl_ctc_fwd(void* stream, const float* logits, const long* gold, const int* in_len, const int* tgt_len, int U, int T, int V, int ld,
                int ldg, int Lmax, int blank, int per_group, float* ws, long ws_bytes, float* nll, float* loss_out) {
    if (!logits || !gold || !in_len || !tgt_len || !ws || !nll || !loss_out) return MTL_EINVAL;
    if (!ctc_dims_ok(U, T, V, Lmax) || ld < V || ldg <= 0 || blank < 0 || blank >= V || per_group <= 0 || U % per_group) return MTL_EINVAL;
    if ((long)U * T > 0x7fffffffL || !ctc_ws_ok(ws, ws_bytes, U, T, Lmax) || ctc_fwd_lds(Lmax) > CTC_LDS_BYTES) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    const int rows = U * T;
    float2* stat = reinterpret_cast<float2*>(ws);
    float* lattice = ws + 2 * (long)rows;
    hipLaunchKernelGGL(ctc_rowstat_kernel, dim3((rows + 3) / 4), dim3(CTC_THREADS), 0, s, logits, rows, V, ld, stat);
    hipLaunchKernelGGL(ctc_alpha_kernel, dim3(U), dim3(CTC_THREADS), (size_t)ctc_fwd_lds(Lmax), s, logits, stat, gold, in_len, tgt_len, T, V,
                       ld, ldg, Lmax, blank, lattice, nll);
    hipLaunchKernelGGL(ctc_loss_kernel, dim3(U / per_group), dim3(CTC_THREADS), 0, s, nll, tgt_len, per_group, Lmax < ldg ? Lmax : ldg,
                       loss_out);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}

int mtl_ctc_bwd(void* stream, const float* logits, const long* gold, const int* in_len, const int* tgt_len, int U, int T, int V, int ld,
                int ldg, int Lmax, int blank, int per_group, const float* ws, long ws_bytes, const float* nll, float gscale,
                const float* gscale_dev, float* dlogits, int ldd) {
    if (!logits || !gold || !in_len || !tgt_len || !ws || !nll || !dlogits) return MTL_EINVAL;
    if (!ctc_dims_ok(U, T, V, Lmax) || ld < V || ldd < V || ldg <= 0 || blank < 0 || blank >= V || per_group <= 0 || U % per_group)
        return MTL_EINVAL;
    if ((long)U * T > 0x7fffffffL || !ctc_ws_ok(ws, ws_bytes, U, T, Lmax) || ctc_bwd_lds(Lmax) > CTC_LDS_BYTES) return MTL_EINVAL;
    hipStream_t s = as_stream(stream);
    const int rows = U * T;
    const float2* stat = reinterpret_cast<const float2*>(ws);
    const float* lattice = ws + 2 * (long)rows;
    hipLaunchKernelGGL(ctc_rows_kernel, dim3((rows + 3) / 4), dim3(CTC_THREADS), 0, s, logits, stat, in_len, tgt_len, nll, rows, T, V, ld,
                       Lmax < ldg ? Lmax : ldg, per_group, gscale, gscale_dev, dlogits, ldd);
    hipLaunchKernelGGL(ctc_beta_kernel, dim3(U), dim3(CTC_THREADS), (size_t)ctc_bwd_lds(Lmax), s, logits, stat, gold, in_len, tgt_len, T, V,
                       ld, ldg, Lmax, blank, lattice, nll, per_group, gscale, gscale_dev, dlogits, ldd);
    MTL_CHECK_LAUNCH();
    return MTL_OK;
}
