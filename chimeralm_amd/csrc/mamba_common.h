// mamba_common.h -- what the Mamba2 kernels of inference (mamba.hip), the running verdict (mamba_verdict.hip) and training
// (mamba_train.hip) state alike, once: constants, conv + SiLU, the fixed-order decay scan, the head's dense layer.  (The B / C chunk
// staging stays a loop of its own in each scan: shared, it cost the d_state-16 inference scan 0.2 - 0.3 % at 4 x 30,000.)
#pragma once
#include "clm_common.h"
#include "mfma32_common.h"

namespace clm {
namespace ssm {

constexpr int P = 64;              // headdim
constexpr int Q = 64;              // scan chunk (tokens)
constexpr int DCONV = 4;
constexpr float EPS = 1e-5f;       // RMSNorm and LayerNorm

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float softplus(float v) { return v > 20.f ? v : log1pf(expf(v)); }   // torch's threshold 20

template <int N>
struct ScanShape {
    static constexpr int NP = N < 32 ? 32 : N;     // state rows held (zero-padded)
    static constexpr int NT = NP / 32;              // 32-row state tiles
    static constexpr int BS = NP + 1;               // B / C row stride (floats): conflict-free column reads
};

// The causal depthwise conv + SiLU of four channels c .. c + 3 of one token: xc[row][c] = silu(b[c] + sum_k w[c][k] zx[row - 3 + k][di + c]),
// rows before the read's start (t = the row's position in its read) counting as zero.
__device__ __forceinline__ void conv4_silu(const float* __restrict__ zx, int ldz, int di, const float* __restrict__ w,
                                           const float* __restrict__ bias, float* __restrict__ xc, int conv_dim, size_t row, int t, int c) {
    f32x4 v = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
    for (int k = 0; k < DCONV; ++k) {
        const int tt = t - (DCONV - 1) + k;
        if (tt >= 0) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(zx + (row - (DCONV - 1) + k) * ldz + di + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += w[(c + e) * DCONV + k] * u[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = silu(v[e]);
    *reinterpret_cast<f32x4*>(xc + row * conv_dim + c) = v;
}

// One chunk's cumulative decay in a fixed-order wave scan: lane i enters with a_i = dt_i A and leaves with s = sum_{k <= i} a_k and
// s63 = the whole chunk's sum.  What becomes of them (exp(s), exp(s63 - s), ...) is each kernel's own.
__device__ __forceinline__ void decay_scan(int lane, float a, float& s, float& s63) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(a, o, 64);
        if (lane >= o) a += u;
    }
    s = a;
    s63 = __shfl(a, 63, 64);
}

// One layer of the head for R rows: acc[r] = bias + sum_c wt[c][o] x[r][c], ascending c, one fmaf chain per (row, output); thread o.
// Each weight is fetched once for the R rows, HEAD_PF of them in flight.  The forward's head runs it with R = 1 and the running
// verdict with R = SSM_VERDICT_ROWS: an interior point is, bit for bit, the arithmetic of a forward of the truncated row.
constexpr int HEAD_PF = 8;
template <int R, int IN>
__device__ __forceinline__ void head_dense(const float* __restrict__ wt, int ldw, int o, float bias, const float (*x)[IN], float* acc) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = bias;
    const float* w = wt + o;
    float wa[HEAD_PF];
#pragma unroll
    for (int j = 0; j < HEAD_PF; ++j) wa[j] = w[(size_t)j * ldw];
#pragma unroll 1
    for (int c0 = 0; c0 < IN; c0 += HEAD_PF) {
        float wc[HEAD_PF];
        const int nx = c0 + HEAD_PF < IN ? c0 + HEAD_PF : 0;     // (wrap-around keeps the prefetch unconditional)
#pragma unroll
        for (int j = 0; j < HEAD_PF; ++j) {
            wc[j] = wa[j];
            wa[j] = w[(size_t)(nx + j) * ldw];
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < HEAD_PF; j += 4) {
                const float4 xv = *reinterpret_cast<const float4*>(&x[r][c0 + j]);
                acc[r] = fmaf(wc[j + 3], xv.w, fmaf(wc[j + 2], xv.z, fmaf(wc[j + 1], xv.y, fmaf(wc[j], xv.x, acc[r]))));
            }
    }
}

}  // namespace ssm
}  // namespace clm
