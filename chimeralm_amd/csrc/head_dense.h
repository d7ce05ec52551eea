// head_dense.h -- one layer of the classifier MLP for HR pooled rows per workgroup (head.hip head_tiles_kernel, trajectory.hip).
// The classifier is a chain of four small matrix-vector products whose cost is the latency of streaming the weights from L2, so:
// every weight element is fetched once per HR rows, each dot product is split in two halves (HEAD_DENSE_THREADS = 1024 threads =
// 512 outputs x 2), and the weight stream runs 16 elements ahead of the FMAs in a register ping-pong.  Weights are transposed
// [in][out]; xin / xout / resid / part are LDS rows of HH floats; the summation order of a row does not depend on HR.
#pragma once
#include "clm_common.h"

namespace clm {

constexpr int HEAD_DENSE_THREADS = 1024;

template <int HR, int IN, bool GELU>
__device__ __forceinline__ void dense_rows(const float* __restrict__ wt, const float* __restrict__ bias,
                                           const float (*xin)[HH], float (*xout)[HH], const float (*resid)[HH],
                                           float (*part)[HH]) {
    constexpr int HALF = IN / 2, PF = 16;
    static_assert(HALF % (2 * PF) == 0, "two prefetch sets per loop trip");
    static_assert(HR % 4 == 0, "rows go four at a time");
    const int o = threadIdx.x & (HH - 1), kh = threadIdx.x >> 9;
    const float* w = wt + (size_t)kh * HALF * HH + o;
    float acc[HR];
#pragma unroll
    for (int r = 0; r < HR; ++r) acc[r] = 0.f;
    float wa[PF], wb[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) wa[j] = w[(size_t)j * HH];
#pragma unroll 1
    for (int i0 = 0; i0 < HALF; i0 += 2 * PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) wb[j] = w[(size_t)(i0 + PF + j) * HH];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rb = 0; rb < HR; rb += 4) {                    // four rows at a time: their x values stay in registers
#pragma unroll
            for (int j = 0; j < PF; j += 4)
#pragma unroll
                for (int r = rb; r < rb + 4; ++r) {
                    const float4 x = *reinterpret_cast<const float4*>(&xin[r][kh * HALF + i0 + j]);
                    acc[r] = fmaf(wa[j + 3], x.w, fmaf(wa[j + 2], x.z, fmaf(wa[j + 1], x.y, fmaf(wa[j], x.x, acc[r]))));
                }
            if constexpr (HR > 4) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int nx = i0 + 2 * PF < HALF ? i0 + 2 * PF : 0;     // wrap-around keeps the prefetch unconditional
#pragma unroll
        for (int j = 0; j < PF; ++j) wa[j] = w[(size_t)(nx + j) * HH];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rb = 0; rb < HR; rb += 4) {                    // four rows at a time: their x values stay in registers
#pragma unroll
            for (int j = 0; j < PF; j += 4)
#pragma unroll
                for (int r = rb; r < rb + 4; ++r) {
                    const float4 x = *reinterpret_cast<const float4*>(&xin[r][kh * HALF + i0 + PF + j]);
                    acc[r] = fmaf(wb[j + 3], x.w, fmaf(wb[j + 2], x.z, fmaf(wb[j + 1], x.y, fmaf(wb[j], x.x, acc[r]))));
                }
            if constexpr (HR > 4) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < HR; ++r) part[r][o] = acc[r];
    }
    __syncthreads();
    if (kh == 0) {
        const float bo = bias[o];
#pragma unroll
        for (int r = 0; r < HR; ++r) {
            float v = (acc[r] + part[r][o]) + bo;
            if (GELU) v = gelu_erf(v);
            if (resid) v += resid[r][o];
            xout[r][o] = v;
        }
    }
    __syncthreads();
}

}  // namespace clm
