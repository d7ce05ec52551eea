// trajectory.hip -- the running verdict: the logits the model would give if a row ended at point k, for every point of every read
// of a chunk, from the pooling partials its forward has already left in HBM (include/chimeralm_hip.h "the running verdict").
//
// Reference arithmetic:
//   BinarySequenceClassifier.forward     /root/reference/chimeralm/models/components/hyena.py:117-146
//     traj[b, k] = classifier(sum_{t < n_k} softmax_{t < n_k}(scores)[t] * ln_f(h[b, t]))   -- the head on the first n_k rows of
//     the final residual stream; the backbone is causal, so those rows do not know what follows them
//
// Three kernels behind stage_head on the forward's stream, no atomics, fixed order: bitwise the same from run to run.
//   1. traj_prefix_kernel      one workgroup per read, one thread per channel: walks the read's tile partials (vec[256], max, sum
//                              per 128- or 64-token tile) in tile order with a RUNNING online softmax and stores vec / sum at
//                              every point boundary.  (head_tiles_kernel scales by the read's global maximum: a prefix whose
//                              scores all lie 90 below a peak behind it would come out as 0 / 0.)  Also finds the read's n_pad.
//   2. traj_classifier_kernel  the classifier chain of head_tiles_kernel (head_dense.h) over the B * (K - 1) interior rows, TRAJ_ROWS = 8
//                              per workgroup: measured against 4 (profiles/trajectory_overhead.txt) the request costs 1.13 against
//                              1.08 ms at 256 x 8,193 and 0.62 against 0.74 ms at 32 x 32,769 -- level, and half the L2 weight stream
//   3. traj_summary_kernel     one thread per read: point K - 1 <- the forward's own logits (bit for bit), then the summary
#include "chimeralm_hip.h"
#include "clm_common.h"
#include "head_dense.h"

namespace clm {

namespace {

constexpr int SEP_ID = 1;         // [SEP] of the reference's tokenizer (the last token of every read)
constexpr int TP_AHEAD = 4;       // tile partials in flight per thread (as head_tiles_kernel)

// partial [B][ntiles][POOL_PSTRIDE]; pooled [B][K][256]; `per` tiles per point (K = ceil(ntiles / per), the last point may be short);
// ids8 [B][Lp] -> npad[b] = length of the leading run of [PAD] (attn_weights.hip's n_pad)
__global__ __launch_bounds__(256) void traj_prefix_kernel(const float* __restrict__ partial, int ntiles, int per, int K,
                                                          float* __restrict__ pooled, const unsigned char* __restrict__ ids8, int L,
                                                          int Lp, int* __restrict__ npad) {
    __shared__ int red[4];
    const int b = blockIdx.x, c = threadIdx.x, lane = c & 63, wave = c >> 6;
    {
        const unsigned char* row = ids8 + (size_t)b * Lp;
        int first = L;
        for (int t = c; t < L; t += 256)
            if (row[t] != PAD_ID) { first = t; break; }      // (ascending t: this thread's first)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        if (lane == 0) red[wave] = first;
        __syncthreads();
        if (c == 0) npad[b] = min(min(red[0], red[1]), min(red[2], red[3]));
    }
    const float* p = partial + (size_t)b * ntiles * POOL_PSTRIDE;
    float* out = pooled + (size_t)b * K * D + c;
    float m = -INFINITY, s = 0.f, v = 0.f;
    float nv[TP_AHEAD];
    float2 nms[TP_AHEAD];
#pragma unroll
    for (int j = 0; j < TP_AHEAD; ++j) {                     // (beyond the read: its last tile again, never used)
        const int i = j < ntiles ? j : ntiles - 1;
        nv[j] = p[(size_t)i * POOL_PSTRIDE + c];
        nms[j] = *reinterpret_cast<const float2*>(p + (size_t)i * POOL_PSTRIDE + D);
    }
    int left = per, k = 0;                                   // tiles left in point k
    for (int i0 = 0; i0 < ntiles; i0 += TP_AHEAD) {
        float cv[TP_AHEAD];
        float2 cms[TP_AHEAD];
#pragma unroll
        for (int j = 0; j < TP_AHEAD; ++j) {
            cv[j] = nv[j];
            cms[j] = nms[j];
            const int i = i0 + TP_AHEAD + j < ntiles ? i0 + TP_AHEAD + j : ntiles - 1;
            nv[j] = p[(size_t)i * POOL_PSTRIDE + c];
            nms[j] = *reinterpret_cast<const float2*>(p + (size_t)i * POOL_PSTRIDE + D);
        }
#pragma unroll
        for (int j = 0; j < TP_AHEAD; ++j) {
            if (i0 + j >= ntiles) break;                     // (uniform)
            const float mn = fmaxf(m, cms[j].x);
            const float a = expf(m - mn), e = expf(cms[j].x - mn);   // (first tile: exp(-inf) = 0)
            s = fmaf(s, a, cms[j].y * e);
            v = fmaf(v, a, cv[j] * e);
            m = mn;
            if ((--left == 0 || i0 + j == ntiles - 1) && k < K) {   // (k < K always: K = ceil(ntiles / per), checked by the host)
                out[(size_t)k * D] = v / s;
                ++k;
                left = per;
            }
        }
    }
}

// rows [n_rows][256] of `pooled` laid out [B][K][256]: row r is read r / (K - 1), point r % (K - 1); logits to traj [B][pstride][2]
__global__ __launch_bounds__(HEAD_DENSE_THREADS) void traj_classifier_kernel(const float* __restrict__ pooled, int K, int n_rows,
                                                                             HeadW hw, float* __restrict__ traj, int64_t pstride) {
    constexpr int R = TRAJ_ROWS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float(*xa)[HH] = reinterpret_cast<float(*)[HH]>(lds);
    float(*xb)[HH] = xa + R;
    float(*xc)[HH] = xb + R;
    float(*part)[HH] = xc + R;
    const int tid = threadIdx.x, r0 = blockIdx.x * R;
    for (int i = tid; i < R * D; i += HEAD_DENSE_THREADS) {
        const int r = i >> 8, c = i & 255, row = r0 + r < n_rows ? r0 + r : n_rows - 1;
        xa[r][c] = pooled[((size_t)(row / (K - 1)) * K + row % (K - 1)) * D + c];
    }
    __syncthreads();
    dense_rows<R, D, true>(hw.w0t, hw.b0, xa, xb, nullptr, part);       // classifier.0 + GELU
    dense_rows<R, HH, true>(hw.w3t, hw.b3, xb, xc, nullptr, part);      // classifier.3 + GELU
    dense_rows<R, HH, true>(hw.w60t, hw.b60, xc, xa, nullptr, part);    // ResidualBlock.layers.0 + GELU
    dense_rows<R, HH, false>(hw.w63t, hw.b63, xa, xb, xc, part);        // ResidualBlock.layers.3 + residual
    if (tid < R * NCLS) {
        const int r = tid / NCLS, cls = tid % NCLS, row = r0 + r;
        if (row < n_rows) {
            float acc = hw.bo[cls];
            for (int i = 0; i < HH; ++i) acc = fmaf(hw.wot[(size_t)i * NCLS + cls], xb[r][i], acc);
            traj[((size_t)(row / (K - 1)) * pstride + row % (K - 1)) * NCLS + cls] = acc;
        }
    }
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.0e38f; }

__global__ __launch_bounds__(64) void traj_summary_kernel(const float* __restrict__ logits, float* __restrict__ traj, int64_t pstride,
                                                          int B, int K, int S, int L, const int* __restrict__ npad,
                                                          const unsigned char* __restrict__ ids8, int Lp,
                                                          clm_traj_summary* __restrict__ summary) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float* t = traj + (size_t)b * pstride * NCLS;
    t[(size_t)(K - 1) * NCLS] = logits[(size_t)b * NCLS];            // the forward's own logits, not recomputed
    t[(size_t)(K - 1) * NCLS + 1] = logits[(size_t)b * NCLS + 1];
    if (!summary) return;
    clm_traj_summary r;
    r.n_pad = npad[b];
    r.has_sep = ids8[(size_t)b * Lp + L - 1] == SEP_ID;
    r.n_bases = max(0, L - r.n_pad - r.has_sep);
    r.n_points = K;
    r.first_k = min(r.n_pad / S, K - 1);                             // first point with n_k > n_pad (an all-[PAD] row: the last)
    const double gap_last = (double)t[(size_t)(K - 1) * NCLS + 1] - (double)t[(size_t)(K - 1) * NCLS];
    r.label = gap_last > 0.0;                                        // a tie (and NaN) is class 0
    r.final_gap = (float)gap_last;
    r.reserved = 0;
    const double sgn = r.label ? 1.0 : -1.0;
    int bad = 0, onset = K - 1, jump = -1;
    bool run = true;                                                 // points [k, K - 1] all carry the final label so far
    double best = 0.0, gap_next = gap_last;
    for (int k = K - 1; k >= r.first_k; --k) {                       // downwards: the onset's run ends at the first other label
        const float l0 = t[(size_t)k * NCLS], l1 = t[(size_t)k * NCLS + 1];
        bad += !(finite_f(l0) && finite_f(l1));
        const double gap = (double)l1 - (double)l0;
        run = run && (gap > 0.0) == (bool)r.label;
        if (run) onset = k;
        if (k < K - 1) {                                             // the step INTO point k + 1
            const double d = sgn * (gap_next - gap);
            if (jump < 0 || d >= best) { best = d; jump = k + 1; }   // (descending k, >=: the lowest k wins a tie)
        }
        gap_next = gap;
    }
    r.n_nonfinite = bad;
    r.onset_k = bad ? -1 : onset;
    r.jump_k = bad ? -1 : jump;
    r.jump_dgap = (bad || jump < 0) ? 0.f : (float)best;
    summary[b] = r;
}

}  // namespace

void launch_traj_prefix(const float* partial, int ntiles, int per, int K, float* pooled, const unsigned char* ids8, int L, int Lp,
                        int* npad, int B, hipStream_t st) {
    hipLaunchKernelGGL(traj_prefix_kernel, dim3(B), dim3(256), 0, st, partial, ntiles, per, K, pooled, ids8, L, Lp, npad);
}

void launch_traj_classifier(const float* pooled, int K, int n_rows, const HeadW& hw, float* traj, int64_t pstride, hipStream_t st) {
    if (n_rows < 1) return;                                  // K = 1: no interior point
    launch_lds<traj_classifier_kernel>(dim3((n_rows + TRAJ_ROWS - 1) / TRAJ_ROWS), dim3(HEAD_DENSE_THREADS),
                                       (size_t)4 * TRAJ_ROWS * HH * sizeof(float), st, pooled, K, n_rows, hw, traj, pstride);
}

void launch_traj_summary(const float* logits, float* traj, int64_t pstride, int B, int K, int S, int L, const int* npad,
                         const unsigned char* ids8, int Lp, clm_traj_summary* summary, hipStream_t st) {
    hipLaunchKernelGGL(traj_summary_kernel, dim3((B + 63) / 64), dim3(64), 0, st, logits, traj, pstride, B, K, S, L, npad, ids8, Lp,
                       summary);
}

}  // namespace clm
