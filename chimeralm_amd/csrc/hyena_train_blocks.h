// hyena_train_blocks.h -- device building blocks of the Hyena training cores: the one-transform op (hyena_train.hip)
// and the segmented op for long reads (hyena_longtrain.hip).  All are __forceinline__ device functions in an
// anonymous namespace: each kernel file gets its own copies and no symbol of its own.
#pragma once
#include "clm_common.h"
#include "fft_passes.h"

namespace clm {
using namespace clmfft;

namespace {

constexpr int HT_PART = 16;                       // floats per (read, channel) of parameter partials: dsw[3][3], dsb[3], dD, 3 unused

// One Stockham pass over the N points in LDS (re / im planes, padded); entered and left with the planes visible to every thread.
template <int LOGN, int R, bool INV>
__device__ __forceinline__ void hyena_train_pass(float* re, float* im, int tid, int Ns, const float2* __restrict__ tw) {
    Cx2 v[16], w[PassGeom<LOGN, R>::NP];
    pass_twiddles<LOGN, R, INV>(w, tid, Ns, tw);
    pass_load<LOGN, R>(re, im, v, tid);
    pass_compute_w<LOGN, R, INV>(v, tid, Ns > 1, w);
    __syncthreads();
    pass_store<LOGN, R>(re, im, v, tid, Ns);
    __syncthreads();
}
// N-point transform in place, natural order in and out, unnormalised in both directions
template <int LOGN, bool INV>
__device__ __forceinline__ void hyena_train_fft(float* re, float* im, int tid, const float2* __restrict__ tw) {
    using P = Plan<LOGN>;
    int Ns = 1;
#pragma unroll
    for (int p = 0; p < P::NPASS - 1; ++p) {
        hyena_train_pass<LOGN, 16, INV>(re, im, tid, Ns, tw);
        Ns *= 16;
    }
    hyena_train_pass<LOGN, P::LAST, INV>(re, im, tid, Ns, tw);
}

// (sum of a, sum of b) over the workgroup, the same value in every thread: lanes in wave_sum's order, waves in wave order.
// `red`: [NT / 64][HT_PART] floats, slots 13 and 14.  Two barriers.
template <int NT>
__device__ __forceinline__ float2 hyena_train_block_sum2(float a, float b, float* red, int tid) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((tid & 63) == 0) red[(tid >> 6) * HT_PART + 13] = a, red[(tid >> 6) * HT_PART + 14] = b;
    __syncthreads();
    float sa = 0.f, sb = 0.f;
    for (int w = 0; w < NT / 64; ++w) sa += red[w * HT_PART + 13], sb += red[w * HT_PART + 14];
    __syncthreads();
    return make_float2(sa, sb);
}
// the power of two that brings a sequence of squared norm n2 to the size of one of squared norm n1 (1 where either is 0 or not finite)
__device__ __forceinline__ float hyena_train_balance(float n1, float n2) {
    if (!(n1 > 0.f) || !(n2 > 0.f) || isinf(n1) || isinf(n2)) return 1.f;
    int sh = (ilogbf(n1) - ilogbf(n2)) / 2;
    sh = sh < -40 ? -40 : (sh > 40 ? 40 : sh);
    return ldexpf(1.f, sh);
}

// The spectrum of two packed real sequences, bin pair (m, N - m) of one thread: S(A2, B2, m) -> the two product spectra S1, S2 at m
// from A2 = 2 A[m], B2 = 2 B[m]; W = S1 + i S2 replaces Z in place.  Bins 0 and N / 2 are their own mirror.
//
// Balance.  The rounding error of a transform is relative to the norm of the WHOLE complex signal, so the smaller of two packed
// sequences keeps only its share of the 24 bits (dc is often 10^5 times smaller than g: packed as they come, dg and dk lost
// four digits).  Each packing therefore scales its imaginary sequence by a power of two -- exact, undone at the end -- that
// brings the two sums of squares within a factor 4: `hyena_train_balance` from the sums, taken in the time domain for the
// inputs and, by Parseval, over the product spectra for the outputs.  The sums come from hyena_train_block_sum2 in one fixed
// order and depend on nothing but the workgroup's own read.
template <int LOGN, class S>
__device__ __forceinline__ float hyena_train_products(float* re, float* im, float* red, int tid, S&& prod) {
    constexpr int N = 1 << LOGN, NT = Plan<LOGN>::NT;
    auto at = [&](int m, int& n, int& pm, int& pn, float2& s1, float2& s2) {
        n = (N - m) & (N - 1), pm = pad_index(m), pn = pad_index(n);
        const float2 zm = make_float2(re[pm], im[pm]), zn = make_float2(re[pn], im[pn]);
        const float2 a2 = make_float2(zm.x + zn.x, zm.y - zn.y);          // Z[m] + conj Z[n]
        const float2 b2 = make_float2(zm.y + zn.y, zn.x - zm.x);          // -i (Z[m] - conj Z[n])
        prod(a2, b2, m, s1, s2);
    };
    float n1 = 0.f, n2 = 0.f;
    for (int m = tid; m <= N / 2; m += NT) {
        int n, pm, pn;
        float2 s1, s2;
        at(m, n, pm, pn, s1, s2);
        const float w = n != m ? 2.f : 1.f;
        n1 = fmaf(w, s1.x * s1.x + s1.y * s1.y, n1);
        n2 = fmaf(w, s2.x * s2.x + s2.y * s2.y, n2);
    }
    const float2 tot = hyena_train_block_sum2<NT>(n1, n2, red, tid);
    const float r = hyena_train_balance(tot.x, tot.y);
    for (int m = tid; m <= N / 2; m += NT) {
        int n, pm, pn;
        float2 s1, s2;
        at(m, n, pm, pn, s1, s2);
        s2.x *= r, s2.y *= r;
        re[pm] = s1.x - s2.y;
        im[pm] = s1.y + s2.x;
        if (n != m) {
            re[pn] = s1.x + s2.y;
            im[pn] = s2.x - s1.y;
        }
    }
    return r;
}

// the imaginary input sequence of this thread's elements times r (after the first loop wrote it unscaled)
template <int LOGN>
__device__ __forceinline__ void hyena_train_scale_im(float* im, int tid, int L, float r) {
    if (r != 1.f)
        for (int t = tid; t < L; t += Plan<LOGN>::NT) im[pad_index(t)] *= r;
}

struct HtTaps {
    float z[3][3];                                // zc[r, t - 2 + j] of the rows x0 | x1 | v
    float u[3];                                   // x0, x1, v at t
};
struct HtShort {                                  // short-filter parameters of one channel's three rows
    float w[3][3], b[3];
    __device__ __forceinline__ void load(const float* __restrict__ sw, const float* __restrict__ sb, int ch) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int e = 0; e < 3; ++e) w[q][e] = sw[(q * D + ch) * 3 + e];
            b[q] = sb[q * D + ch];
        }
    }
};
// rows of a read begin at 4 L bytes: every access is a 4-byte one
__device__ __forceinline__ void hyena_train_taps(const float* __restrict__ zb, int ch, int t, int L, const HtShort& s, HtTaps& o) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float* row = zb + (size_t)(q * D + ch) * L;
        o.z[q][0] = t >= 2 ? row[t - 2] : 0.f;
        o.z[q][1] = t >= 1 ? row[t - 1] : 0.f;
        o.z[q][2] = row[t];
        o.u[q] = fmaf(s.w[q][2], o.z[q][2], fmaf(s.w[q][1], o.z[q][1], fmaf(s.w[q][0], o.z[q][0], s.b[q])));
    }
}

}  // namespace
}  // namespace clm
