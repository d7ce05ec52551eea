// mfma32_common.h -- the 64-token tile machinery of the exact-fp32 / fp16x3 kernels, shared as device code by tail32.hip (Hyena
// tail, transformer encoder and stem, DNAConvNet) and mamba.hip (Mamba2 projections): tile geometry, the packed weight-set pipeline,
// the two arithmetics (AR_F32 / AR_X3), the convolutions' input staging (stage_rows) and the MFMA loops.  Moved out of tail32.hip
// unchanged; see the comments there for the design.
#pragma once
#include "clm_common.h"

namespace clm {

namespace {

constexpr int BM32 = 64;          // tokens per tile
constexpr int RS32 = 260;         // row stride (floats) of the token-major tiles: 1040 B -- the 16 rows of a ds_read_b128 lane group
                                  // fall on 16 different 16-byte bank groups (260 = 4 mod 64)
constexpr int RSY = 72;           // row stride (floats) of the k-major y tile: the two half-waves of an MFMA read rows k and k + 4, i.e. 288 floats = banks + 32
constexpr int KS_SET = 8;         // k-steps (of 8) per weight set: 64 deep

using f32x4 = float __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const f32x4* wset_ptr(const f32x4* wp, int nb, int ksteps_all, int ks0, int wave, int lane) {
    return wp + ((size_t)(nb * 8 + wave) * ksteps_all + ks0) * 64 + lane;
}
__device__ __forceinline__ void load_wset(const f32x4* p, f32x4 (&ws)[KS_SET]) {
#pragma unroll
    for (int s = 0; s < KS_SET; ++s) ws[s] = p[(size_t)s * 64];
}
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---- ARITH: the arithmetic of the products.  AR_F32: exact fp32 on v_mfma_f32_32x32x2_f32.  AR_X3 ("fp16x3"): every operand split
// into two halfs, x = hi + lo with hi = fp16(x), lo = fp16(x - hi) (~21 bits), and a product as THREE fp16 MFMAs into the fp32
// accumulator -- w_hi a_hi + w_lo a_hi + w_hi a_lo (the dropped w_lo a_lo is 2^-22 of the product) -- at 96 cycles per 16-deep step
// and row tile where the fp32 MFMA takes 512.  A tile row then holds 256 hi halfs | 256 lo halfs in the 1024 bytes of its 256
// floats (same stride, same bank behaviour); a weight "fragment" is 8 halfs, (hi, lo) pairs alternating, so a 64-deep set is again
// 8 fragments of 16 bytes and the set machinery is shared.  Weights are packed x 2^10 (X3_WS), which keeps their lo halfs out of
// fp16's subnormal range down to |w| ~ 2.5e-4; accumulators that also hold unscaled terms (the residual) are scaled before and
// unscaled after their products (powers of two: exact).
enum { AR_F32 = 0, AR_X3 = 1 };
constexpr float X3_WS = 1024.f, X3_WSI = 1.0f / 1024.f;
template <int AR> constexpr float WSCALE = AR == AR_X3 ? X3_WS : 1.0f;
template <int AR> constexpr float WUNSCALE = AR == AR_X3 ? X3_WSI : 1.0f;
using v4i16 = short __attribute__((ext_vector_type(4)));
typedef v4i16 __attribute__((address_space(3))) * lds_v4i16_ptr32;
constexpr int RSKM64 = 96;        // AR_X3: row stride (halfs) of a k-major y plane [256 channels][64 tokens]: 192 B -- the four rows of a
                                  // transposing read fall on four different 64-byte bank groups (0, 192, 128, 64 mod 256)

__device__ __forceinline__ f32x16 mfma16(f32x4 a, f32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// x -> (hi, lo) halfs.  Values beyond fp16's range do not become inf: hi saturates at +-65504 and lo carries the rest (up to twice
// the range; beyond that the pair saturates) -- the mode has no guard, so an outlier must not turn into a NaN logit.
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 clamp_h(f32x4 v) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = __builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
    return r;
}
__device__ __forceinline__ void split4(f32x4 v, h4_t& hi, h4_t& lo) {
    hi = __builtin_convertvector(clamp_h(v), h4_t);
    lo = __builtin_convertvector(clamp_h(v - __builtin_convertvector(hi, f32x4)), h4_t);
}
// four consecutive features of one token row into a tile (fp32: 16 bytes; x3: 8 bytes of hi halfs + 8 bytes of lo halfs)
template <int AR>
__device__ __forceinline__ void tile_store4(float* T, int row, int col, f32x4 v) {
    if constexpr (AR == AR_F32) {
        *reinterpret_cast<f32x4*>(T + row * RS32 + col) = v;
    } else {
        h4_t hi, lo;
        split4(v, hi, lo);
        char* base = reinterpret_cast<char*>(T + row * RS32) + col * 2;
        *reinterpret_cast<h4_t*>(base) = hi;
        *reinterpret_cast<h4_t*>(base + 512) = lo;
    }
}
// The implicit-GEMM convolutions' input tile: rows t0 - HALO .. t0 + 63 + HALO of one read x [Lin][256] -> Xs rows 0 .. 63 + 2 HALO,
// zero outside [0, Lin): a wave per row, 16 bytes per lane, the eight waves in nine trips (the taps then read Xs shifted by rows)
template <int AR, int HALO>
__device__ __forceinline__ void stage_rows(float* Xs, const float* __restrict__ x, int t0, int Lin, int wave, int lane) {
    const float* src = x + lane * 4;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int r = wave + 8 * i, t = t0 - HALO + r;
        if (r < BM32 + 2 * HALO) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t >= 0 && t < Lin) v = *reinterpret_cast<const f32x4*>(src + (size_t)t * D);
            tile_store4<AR>(Xs, r, lane * 4, v);
        }
    }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
}

// acc[mt] += W-set x T[tokens mt*32.., k = 64 part ..): token-major tile
template <int AR>
__device__ __forceinline__ void compute_set_tm(const float* T, int part, int lrow, int lhalf, const f32x4 (&ws)[KS_SET], f32x16 (&acc)[2]) {
    if constexpr (AR == AR_X3) {
        // (the fragments of item i + 2 requested before the MFMAs of item i, pinned with sched_group_barrier, was measured: 4,121 vs
        //  4,180 reads/s on the Hyena path, 7,269 vs 7,637 on the transformer -- no gain over what hipcc schedules; the simple form stays)
        const char* a0 = reinterpret_cast<const char*>(T + lrow * RS32) + (part * 64 + lhalf * 8) * 2;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const f32x4 ah = *reinterpret_cast<const f32x4*>(a0 + mt * 32 * RS32 * 4 + s * 32);
                const f32x4 al = *reinterpret_cast<const f32x4*>(a0 + 512 + mt * 32 * RS32 * 4 + s * 32);
                acc[mt] = mfma16(ws[2 * s], ah, acc[mt]);
                acc[mt] = mfma16(ws[2 * s + 1], ah, acc[mt]);
                acc[mt] = mfma16(ws[2 * s], al, acc[mt]);
            }
        return;
    }
    const float* a0 = T + lrow * RS32 + part * 64 + lhalf * 4;
    f32x4 af[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) af[0][mt] = *reinterpret_cast<const f32x4*>(a0 + mt * 32 * RS32);
#pragma unroll
    for (int s = 0; s < KS_SET; ++s) {
        if (s + 1 < KS_SET) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) af[(s + 1) & 1][mt] = *reinterpret_cast<const f32x4*>(a0 + mt * 32 * RS32 + (s + 1) * 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt] = mfma32(ws[s][j], af[s & 1][mt][j], acc[mt]);
    }
}
// same from the k-major tile (out_proj: y is channel-major).  fp32: Ys[k][token] floats; x3: two planes of halfs [k][RSKM64] read with
// the transposing LDS read (a 16-lane group reads a 4(k) x 16(token) block, lane i receives token i's four k values)
template <int AR>
__device__ __forceinline__ void compute_set_km(const float* Ys, int part, int lane, const f32x4 (&ws)[KS_SET], f32x16 (&acc)[2]) {
    const int lrow = lane & 31, lhalf = lane >> 5;
    if constexpr (AR == AR_X3) {
        const unsigned short* Yh = reinterpret_cast<const unsigned short*>(Ys);
        const int li = lane & 15, g1 = (lane >> 4) & 1, q = li >> 2, p = li & 3;
        const unsigned short* base = Yh + (8 * lhalf + q) * RSKM64 + 16 * g1 + 4 * p;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const unsigned short* p0 = base + ((part * 4 + s) * 16) * RSKM64 + mt * 32;
                f32x4 a2[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const unsigned short* pp = p0 + pl * (D * RSKM64);
                    const v4i16 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr32)(pp));
                    const v4i16 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr32)(pp + 4 * RSKM64));
                    typedef short s8 __attribute__((ext_vector_type(8)));
                    const s8 both = {l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
                    a2[pl] = __builtin_bit_cast(f32x4, both);
                }
                acc[mt] = mfma16(ws[2 * s], a2[0], acc[mt]);
                acc[mt] = mfma16(ws[2 * s + 1], a2[0], acc[mt]);
                acc[mt] = mfma16(ws[2 * s], a2[1], acc[mt]);
            }
        return;
    }
    const float* a0 = Ys + (part * 64 + lhalf * 4) * RSY + lrow;
#pragma unroll
    for (int s = 0; s < KS_SET; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt] = mfma32(ws[s][j], a0[(s * 8 + j) * RSY + mt * 32], acc[mt]);
}

// one 256-deep product: sets 0..3 starting at fragment ks0 of (wp, nb); ws[0] holds set 0 on entry, and on exit the first set of
// what follows (`nxt`, requested under the last set: unconditional)
template <bool KM, int AR = AR_F32>
__device__ __forceinline__ void product256(const float* T, const f32x4* wp, int nb, int ksteps_all, int ks0, const f32x4* nxt,
                                           int wave, int lane, f32x4 (&ws)[2][KS_SET], f32x16 (&acc)[2]) {
    const int lrow = lane & 31, lhalf = lane >> 5;
    static_for<0, 4>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        if constexpr (p < 3) load_wset(wset_ptr(wp, nb, ksteps_all, ks0 + (p + 1) * KS_SET, wave, lane), ws[(p + 1) & 1]);
        else load_wset(nxt, ws[0]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (KM) compute_set_km<AR>(T, p, lane, ws[p & 1], acc);
        else compute_set_tm<AR>(T, p, lrow, lhalf, ws[p & 1], acc);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// acc[mt] += W x of the token-major tile T, 256 deep: product256's arithmetic on the same packed fragments (launch_pack_f32t; k-step
// ks = fragment ks of this wave at wp), but with a ring of four fragments requested four k-steps (2,048 MFMA cycles) ahead instead of
// product256's two 64-deep sets: those are 64 registers, which a kernel with other accumulators to hold does not have
// (pool_train.hip: the 128 of dW1; cnn_train.hip: one accumulator per tap and their sum)
__device__ __forceinline__ void product256_ring(const float* T, const f32x4* wp, int lrow, int lhalf, f32x16 (&acc)[2]) {
    f32x4 w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = wp[(size_t)i * 64];
    const float* a0 = T + lrow * RS32 + lhalf * 4;
#pragma unroll 1
    for (int s4 = 0; s4 < D / 8; s4 += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 af0 = *reinterpret_cast<const f32x4*>(a0 + (s4 + i) * 8);
            const f32x4 af1 = *reinterpret_cast<const f32x4*>(a0 + 32 * RS32 + (s4 + i) * 8);
            const f32x4 wc = w[i];
            const int nx = s4 + 4 + i < D / 8 ? s4 + 4 + i : i;      // (wrap-around keeps the request unconditional)
            w[i] = wp[(size_t)nx * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = mfma32(wc[j], af0[j], acc[0]);
                acc[1] = mfma32(wc[j], af1[j], acc[1]);
            }
        }
    }
}

// LayerNorm over the 256 features of the 64 tokens in accumulator layout (rows = this wave's 32 features, lane = token) -> T
// (fp32, token-major); two-pass statistics like every fp32 LayerNorm of the engine (gemm_common.h stage_a_tile).  Ends with a
// barrier (T complete); its first barrier also orders every earlier LDS read of the workgroup before the writes.
// KEEP: the normalised values also replace the accumulator contents (post-norm blocks: they are the next residual).
template <bool KEEP = false, int AR = AR_F32>
__device__ __forceinline__ void ln_to_tile(f32x16 (&acc)[2], float* P1, float* P2, const float* __restrict__ g,
                                           const float* __restrict__ bta, float eps, float* T, int valid, int wave, int lrow, int lhalf) {
    float mean[2], rstd[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[mt][r];
        s += __shfl_xor(s, 32, 64);
        if (lhalf == 0) P1[wave * BM32 + mt * 32 + lrow] = s;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += P1[w * BM32 + mt * 32 + lrow];
        mean[mt] = s * (1.0f / D);
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = acc[mt][r] - mean[mt];
            v += d * d;
        }
        v += __shfl_xor(v, 32, 64);
        if (lhalf == 0) P2[wave * BM32 + mt * 32 + lrow] = v;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += P2[w * BM32 + mt * 32 + lrow];
        rstd[mt] = 1.0f / sqrtf(v * (1.0f / D) + eps);
    }
    const float* gp = g + wave * 32 + 4 * lhalf;
    const float* bp = bta + wave * 32 + 4 * lhalf;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 g4 = *reinterpret_cast<const float4*>(gp + 8 * q);
        const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * q);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const bool ok = mt * 32 + lrow < valid;          // rows beyond the read leave as zeros
            f32x4 y;
            y[0] = ok ? (acc[mt][4 * q + 0] - mean[mt]) * rstd[mt] * g4.x + b4.x : 0.f;
            y[1] = ok ? (acc[mt][4 * q + 1] - mean[mt]) * rstd[mt] * g4.y + b4.y : 0.f;
            y[2] = ok ? (acc[mt][4 * q + 2] - mean[mt]) * rstd[mt] * g4.z + b4.z : 0.f;
            y[3] = ok ? (acc[mt][4 * q + 3] - mean[mt]) * rstd[mt] * g4.w + b4.w : 0.f;
            if constexpr (KEEP) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[mt][4 * q + e] = y[e];
            }
            tile_store4<AR>(T, mt * 32 + lrow, wave * 32 + 8 * q + 4 * lhalf, y);
        }
    }
    __syncthreads();
}

}  // namespace

}  // namespace clm
