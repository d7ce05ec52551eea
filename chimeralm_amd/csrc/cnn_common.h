// cnn_common.h -- what DNAConvNet's inference (cnn.hip, tail32.hip's cnn_gemm7_kernel) and training (cnn_train.hip) kernels share:
// the net's constants and block 0's two LDS staging steps (the tap table and the window's table rows).
#pragma once
#include "clm_common.h"

namespace clm {
namespace cnn {

constexpr int VOC = 12;            // embedding rows
constexpr int K = 7, HALO = 3;     // taps, "same" padding on each side
constexpr int TROWS = VOC + 1;     // LDS table rows per tap: the 12 ids + a zero row for positions outside the read
constexpr float BN_EPS = 1e-5f;

// Block 0, 512 threads: the tap table T [K][VOC][256] -> LDS Ts [K][TROWS][256], row VOC of every tap zero
__device__ __forceinline__ void stage_table(float* Ts, const float* __restrict__ table, int tid) {
    for (int i = tid; i < K * TROWS * D / 4; i += 512) {
        const int row = i / (D / 4), dk = row / TROWS, tok = row % TROWS, c4 = i % (D / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tok < VOC) v = *reinterpret_cast<const float4*>(table + ((size_t)dk * VOC + tok) * D + 4 * c4);
        *reinterpret_cast<float4*>(Ts + (size_t)row * D + 4 * c4) = v;
    }
}
// Block 0, 512 threads: idl[i] = scale x the table row of token first + i of the read `ids` [L], i < n (scale 1: the row, D: its LDS
// offset).  Outside [0, L): the zero row; ids past the vocabulary clamp to its last row (ids8 holds [0, 16)).
__device__ __forceinline__ void stage_token_rows(int* idl, const unsigned char* __restrict__ ids, int first, int n, int L, int tid, int scale) {
    for (int i = tid; i < n; i += 512) {
        const int t = first + i;
        int id = VOC;
        if (t >= 0 && t < L) {
            id = ids[t];
            id = id < VOC ? id : VOC - 1;
        }
        idl[i] = id * scale;
    }
}

}  // namespace cnn
}  // namespace clm
