// mamba_verdict.hip -- the running verdict of the two Mamba nets: the logits the model would give if a row ended at point k, for
// every point of every read of a chunk, from the pooling partials its forward has already left in HBM (include/chimeralm_hip.h
// "the running verdict of the Mamba nets").
//
// Reference arithmetic (the reference's chimeralm/models/components/mamba.py, both classes):
//   traj[b, k] = classifier(pooler((mean_{t < n_k} h[b, t] + max_{t < n_k} h[b, t]) / 2))
// Embedding, positional term, mask, causal convolution, scan from a zero state and per-token RMSNorm are all causal, so h[b, t] of
// the whole row IS h[b, t] of the row cut anywhere behind t; the mean and the maximum of a prefix are a running sum and a running
// maximum over the per-64-token partials mamba_proj_kernel<EPI_OUTPOOL> writes (part [reads][tiles][2][d]: sums | maxima).
//
// Two kernels behind mamba_head_kernel on the forward's stream, then trajectory.hip's summary kernel; no atomics, fixed order:
// bitwise the same from run to run.
//   1. ssm_verdict_pool_kernel  one workgroup per read, one thread per channel: walks the read's tile partials in tile order
//                               (s += sum_i as mamba_head_kernel, a running fmaxf) and stores (s / n_k + mx) / 2 at every point
//                               boundary.  Also finds the read's n_pad.
//   2. ssm_verdict_head_kernel  pooler, classifier.0 and classifier.3 of mamba_head_kernel over the reads x (K - 1) interior rows,
//                               SSM_VERDICT_ROWS per workgroup: each weight of the two d-wide matrices is fetched once per group of
//                               rows.  The d-wide layers are mamba_common.h's head_dense, the routine mamba_head_kernel runs on its
//                               one row (bias first, fmaf over ascending input index): an interior point is the arithmetic of a
//                               forward of the truncated row.
#include "chimeralm_hip.h"
#include "clm_common.h"
#include "mamba_common.h"

namespace clm {

namespace {

constexpr int VP_AHEAD = 4;       // tile partials in flight per thread (as traj_prefix_kernel)

// part [reads][tiles][2][d]; pooled [reads][K][d]; `per` tiles per point (K = ceil(L / S), S = 64 per; the last point may be short and
// may end in a partial tile); ids8 [reads][Lp] -> npad[b] = length of the leading run of [PAD]
__global__ __launch_bounds__(512) void ssm_verdict_pool_kernel(const float* __restrict__ part, int tiles, int per, int K, int L, int d,
                                                               float* __restrict__ pooled, const unsigned char* __restrict__ ids8,
                                                               int Lp, int* __restrict__ npad) {
    __shared__ int red[8];
    const int b = blockIdx.x, c = threadIdx.x, lane = c & 63, wave = c >> 6, nwaves = d >> 6;
    {
        const unsigned char* row = ids8 + (size_t)b * Lp;
        int first = L;
        for (int t = c; t < L; t += d)
            if (row[t] != PAD_ID) { first = t; break; }      // (ascending t: this thread's first)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        if (lane == 0) red[wave] = first;
        __syncthreads();
        if (c == 0) {
            int f = red[0];
            for (int w = 1; w < nwaves; ++w) f = min(f, red[w]);
            npad[b] = f;
        }
    }
    const size_t ts = (size_t)2 * d;                         // floats per tile partial
    const float* p = part + (size_t)b * tiles * ts + c;
    float* out = pooled + (size_t)b * K * d + c;
    float s = 0.f, mx = -INFINITY;
    float ns[VP_AHEAD], nm[VP_AHEAD];
#pragma unroll
    for (int j = 0; j < VP_AHEAD; ++j) {                     // (beyond the read: its last tile again, never used)
        const int i = j < tiles ? j : tiles - 1;
        ns[j] = p[(size_t)i * ts];
        nm[j] = p[(size_t)i * ts + d];
    }
    int left = per, k = 0;                                   // tiles left in point k
    for (int i0 = 0; i0 < tiles; i0 += VP_AHEAD) {
        float cs[VP_AHEAD], cm[VP_AHEAD];
#pragma unroll
        for (int j = 0; j < VP_AHEAD; ++j) {
            cs[j] = ns[j];
            cm[j] = nm[j];
            const int i = i0 + VP_AHEAD + j < tiles ? i0 + VP_AHEAD + j : tiles - 1;
            ns[j] = p[(size_t)i * ts];
            nm[j] = p[(size_t)i * ts + d];
        }
#pragma unroll
        for (int j = 0; j < VP_AHEAD; ++j) {
            if (i0 + j >= tiles) break;                      // (uniform)
            s += cs[j];
            mx = fmaxf(mx, cm[j]);
            if ((--left == 0 || i0 + j == tiles - 1) && k < K) {   // (k < K always: K = ceil(tiles / per), checked by the host)
                const int n_k = min((k + 1) * per * 64, L);  // tokens point k covers
                out[(size_t)k * d] = (s / (float)n_k + mx) * 0.5f;
                ++k;
                left = per;
            }
        }
    }
}

// rows [n_rows][DV] of `pooled` laid out [reads][K][DV]: row r is read r / (K - 1), point r % (K - 1); logits to traj [reads][pstride][2]
template <int DV>
__global__ __launch_bounds__(DV) void ssm_verdict_head_kernel(const float* __restrict__ pooled, int K, int n_rows,
                                                              const float* __restrict__ wpt, const float* __restrict__ bp,
                                                              const float* __restrict__ w0t, const float* __restrict__ b0,
                                                              const float* __restrict__ w3, const float* __restrict__ b3,
                                                              float* __restrict__ traj, int64_t pstride) {
    constexpr int R = SSM_VERDICT_ROWS, D2 = DV / 2;
    __shared__ __attribute__((aligned(16))) float Pv[R][DV];
    __shared__ __attribute__((aligned(16))) float X1[R][DV];
    __shared__ __attribute__((aligned(16))) float X2[R][D2];
    const int tid = threadIdx.x, r0 = blockIdx.x * R;
#pragma unroll
    for (int r = 0; r < R; ++r) {                            // (beyond the last row: the last row again, never written)
        const int row = r0 + r < n_rows ? r0 + r : n_rows - 1;
        Pv[r][tid] = pooled[((size_t)(row / (K - 1)) * K + row % (K - 1)) * DV + tid];
    }
    __syncthreads();
    float acc[R];
    ssm::head_dense<R, DV>(wpt, DV, tid, bp[tid], Pv, acc);                     // pooler.0 + GELU
#pragma unroll
    for (int r = 0; r < R; ++r) X1[r][tid] = gelu_erf(acc[r]);
    __syncthreads();
    if (tid < D2) {
        ssm::head_dense<R, DV>(w0t, D2, tid, b0[tid], X1, acc);                 // classifier.0 + GELU
#pragma unroll
        for (int r = 0; r < R; ++r) X2[r][tid] = gelu_erf(acc[r]);
    }
    __syncthreads();
    if (tid < R * NCLS) {                                                     // classifier.3 (mamba_head_kernel: the bias last)
        const int r = tid / NCLS, cls = tid % NCLS, row = r0 + r;
        if (row < n_rows) {
            float a = 0.f;
            for (int c = 0; c < D2; ++c) a = fmaf(w3[(size_t)cls * D2 + c], X2[r][c], a);
            traj[((size_t)(row / (K - 1)) * pstride + row % (K - 1)) * NCLS + cls] = a + b3[cls];
        }
    }
}

}  // namespace

void launch_ssm_verdict_pool(const float* part, int tiles, int per, int K, int L, int d, float* pooled, const unsigned char* ids8, int Lp,
                             int* npad, int reads, hipStream_t st) {
    hipLaunchKernelGGL(ssm_verdict_pool_kernel, dim3(reads), dim3(d), 0, st, part, tiles, per, K, L, d, pooled, ids8, Lp, npad);
}

void launch_ssm_verdict_head(const float* pooled, int K, int n_rows, int d, const float* wpt, const float* bp, const float* w0t,
                             const float* b0, const float* w3, const float* b3, float* traj, int64_t pstride, hipStream_t st) {
    if (n_rows < 1) return;                                  // K = 1: no interior point
    const dim3 grid((n_rows + SSM_VERDICT_ROWS - 1) / SSM_VERDICT_ROWS);
    hipLaunchKernelGGL(d == 256 ? ssm_verdict_head_kernel<256> : ssm_verdict_head_kernel<512>, grid, dim3(d), 0, st, pooled, K, n_rows, wpt,
                       bp, w0t, b0, w3, b3, traj, pstride);
}

}  // namespace clm
