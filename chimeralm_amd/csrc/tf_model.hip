// tf_model.hip -- SequenceCNNTransformer forward on MI355X: kernels + engine + C ABI.
//
// Reference: /root/reference/chimeralm/models/components/transformer.py
//   :28-86  modules   Embedding(12, 256, padding_idx 4) ; 3 x [Conv1d(256, 256, k=3, padding=1), ReLU, MaxPool1d(2, 2)] ;
//                     SinusoidalPositionalEncoding ; LayerNorm ; TransformerEncoder(12 x post-norm layer: 8 heads of 32,
//                     feed-forward 1024, ReLU) ; Linear(256, 1) softmax pooling ; Linear(256, 128), ReLU, Linear(128, 2)
//   :88-104 forward   (no masks anywhere: pads are ordinary tokens)
// configured by /root/reference/configs/model/transformer.yaml:3-12.  Oracle: oracle/transformer_oracle.py (pinned against the
// reference module itself, tests/golden/transformer_golden.npz).
//
// First correct version: every stage is its own kernel (the Hyena path's fusion lessons are not applied yet); the dense work is
// on MFMA with the same LDS-resident 128-token activation tile / register-resident weight half-set scheme as gemm16.hip, the
// attention is attention.hip.  Data layout, one batch of B reads (L tokens -> L3 = L / 8 positions, M = B * L3 rows):
//   x1 [B, L/2, 256], x2 [B, L/4, 256], x3 [B, L3, 256]     16-bit, token-major          conv stack
//   h  [M, 256] fp32 (residual stream, post-norm: always a LayerNorm output)   hx [M, 256] 16-bit copy = next GEMM operand
//   qkv [M, 768], att [M, 256]                               16-bit
// The convolution is a GEMM with K = 3 * 256: one 130-row tile of the input (1 halo row each side) feeds three passes with the
// row offset 0 / 1 / 2 and the weight slice W[:, :, dk]; ReLU and the max-pool happen on the accumulator quads (4 consecutive
// positions of one channel) before anything is written.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "chimeralm_hip.h"
#include "gemm16_common.h"
#include "handle_host.h"

namespace clm {
namespace tf {

constexpr int TFF = 1024, TQKV = 768, TVOC = 12, TCH = 128 /* classifier hidden */;
constexpr int ZRS = 40;   // row stride (elements) of the wave-private [token][32 features] output staging tiles: 80 bytes

// ------------------------------------------------------------------------------------------------ small helpers
__global__ void conv_w_split_kernel(const float* __restrict__ w, float* __restrict__ out) {   // [co][ci][3] -> [3][co][ci]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * D * 3) return;
    const int dk = i % 3, ci = (i / 3) % D, co = i / (3 * D);
    out[((size_t)dk * D + co) * D + ci] = w[i];
}

// wave-private [128 tokens][32 features] 16-bit tile -> global rows (64 bytes per token and wave), 16 rows per instruction
template <typename E>
__device__ __forceinline__ void store_wave_tile(const E* zs, E* out, size_t row0, size_t nrows_valid, int ld, int col0, int lane,
                                                int ntok) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = i * 16 + (lane >> 2), piece = lane & 3;
        if (row < ntok && (size_t)row < nrows_valid) {
            const uint4 v = *reinterpret_cast<const uint4*>(zs + row * ZRS + piece * 8);
            *reinterpret_cast<uint4*>(out + (row0 + row) * ld + col0 + piece * 8) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ conv + ReLU + max-pool
template <int PREC, bool FROM_IDS>
__global__ __launch_bounds__(512) void conv3_relu_pool_kernel(const unsigned char* __restrict__ ids8, int ids_stride,
                                                              const float* __restrict__ emb,
                                                              const typename CT<PREC>::elem* __restrict__ xin,
                                                              const void* __restrict__ wpk, const float* __restrict__ bias,
                                                              typename CT<PREC>::elem* __restrict__ xout, int Lin, int Lout) {
    using elem = typename CT<PREC>::elem;
    using frag = u16x8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    elem* As = reinterpret_cast<elem*>(smem);                 // [130][RS16]: input rows t0 - 1 .. t0 + 128
    elem* Zs = As + 130 * RS16;                               // 8 x [64 pooled positions][ZRS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * 128;
    const frag* wp = reinterpret_cast<const frag*>(wpk);
    constexpr size_t WSLICE = (size_t)D * D / 8 * WFR<PREC>;  // fragments per [256 x 256] slice
    f32x16 acc[4];
    frag bs[2][1][SETK];
    load_set<PREC, D, 1>(wp, 0, 0, 0, wave, lane, bs[0]);
    __builtin_amdgcn_sched_barrier(0);
    {
        const int piece = tid & 31;
#pragma unroll 1
        for (int r = tid >> 5; r < 130; r += 16) {
            const int tg = t0 - 1 + r;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (tg >= 0 && tg < Lin) {
                if (FROM_IDS) {
                    const int id = ids8[(size_t)b * ids_stride + tg];
                    const float* e = emb + (size_t)(id < TVOC ? id : TVOC - 1) * D + piece * 8;
                    const float4 a = *reinterpret_cast<const float4*>(e), c4 = *reinterpret_cast<const float4*>(e + 4);
                    u16x8 pk = {to_bits<PREC>(a.x), to_bits<PREC>(a.y), to_bits<PREC>(a.z), to_bits<PREC>(a.w),
                                to_bits<PREC>(c4.x), to_bits<PREC>(c4.y), to_bits<PREC>(c4.z), to_bits<PREC>(c4.w)};
                    v = __builtin_bit_cast(uint4, pk);
                } else {
                    v = *reinterpret_cast<const uint4*>(xin + ((size_t)b * Lin + tg) * D + piece * 8);
                }
            }
            *reinterpret_cast<uint4*>(As + r * RS16 + piece * 8) = v;
        }
    }
    __syncthreads();
    zero_acc(acc);
#pragma unroll
    for (int dk = 0; dk < 3; ++dk)                            // y[t] += W[:, :, dk] x[t + dk - 1]
        phase_tm<PREC, D, D, false>(As + dk * RS16, wp + dk * WSLICE, 0, 0, wp + (dk < 2 ? dk + 1 : 0) * WSLICE, 0, 0, wave, lane, bs,
                                    acc);
    // rows = positions (register quads = 4 consecutive positions), lane = output channel wave*32 + lrow
    elem* zs = Zs + wave * 64 * ZRS;
    const float bv = bias[wave * 32 + lrow];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float v0 = fmaxf(acc[mt][4 * g + 0] + bv, 0.f), v1 = fmaxf(acc[mt][4 * g + 1] + bv, 0.f);
            const float v2 = fmaxf(acc[mt][4 * g + 2] + bv, 0.f), v3 = fmaxf(acc[mt][4 * g + 3] + bv, 0.f);
            const int pl = 16 * mt + 4 * g + 2 * lhalf;       // pooled position inside the tile
            zs[pl * ZRS + lrow] = from_float<elem>(fmaxf(v0, v1));
            zs[(pl + 1) * ZRS + lrow] = from_float<elem>(fmaxf(v2, v3));
        }
    const size_t p0 = (size_t)(t0 / 2);
    const size_t valid = (size_t)Lout > p0 ? (size_t)Lout - p0 : 0;
    store_wave_tile<elem>(zs, xout + (size_t)b * Lout * D, p0, valid, D, wave * 32, lane, 64);
}

// ------------------------------------------------------------------------------------------------ + PE, LayerNorm
template <int PREC>
__global__ __launch_bounds__(256) void pe_ln_kernel(const typename CT<PREC>::elem* __restrict__ x, const float* __restrict__ pe,
                                                    const float* __restrict__ g, const float* __restrict__ bta,
                                                    float* __restrict__ h, typename CT<PREC>::elem* __restrict__ hx,
                                                    size_t M, int L3, float eps) {
    using elem = typename CT<PREC>::elem;
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int t = (int)(row % (size_t)L3);
    const u16x4 raw = *reinterpret_cast<const u16x4*>(x + row * D + lane * 4);
    const float4 p = *reinterpret_cast<const float4*>(pe + (size_t)t * D + lane * 4);
    elem e0, e1, e2, e3;
    e0.bits = raw[0]; e1.bits = raw[1]; e2.bits = raw[2]; e3.bits = raw[3];
    const float x0 = to_float(e0) + p.x, x1 = to_float(e1) + p.y, x2 = to_float(e2) + p.z, x3 = to_float(e3) + p.w;
    const float mean = wave_sum((x0 + x1) + (x2 + x3)) * (1.0f / D);
    const float d0 = x0 - mean, d1 = x1 - mean, d2 = x2 - mean, d3 = x3 - mean;
    const float var = wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.0f / D);
    const float rstd = 1.0f / sqrtf(var + eps);
    const float4 g4 = *reinterpret_cast<const float4*>(g + lane * 4), b4 = *reinterpret_cast<const float4*>(bta + lane * 4);
    const float y0 = d0 * rstd * g4.x + b4.x, y1 = d1 * rstd * g4.y + b4.y, y2 = d2 * rstd * g4.z + b4.z,
                y3 = d3 * rstd * g4.w + b4.w;
    *reinterpret_cast<float4*>(h + row * D + lane * 4) = make_float4(y0, y1, y2, y3);
    store4<elem>(hx + row * D + lane * 4, y0, y1, y2, y3);
}

// ------------------------------------------------------------------------------------------------ dense layers
struct LinArgs {
    const void* a;            // [M, K] 16-bit, token-major
    const void* w;            // packed [N, K]
    const float* bias;        // [N]
    void* out16;              // [M, N] 16-bit
    size_t M;
    int relu;
};
enum { E_ACT = 0 };           // bias (+ ReLU) -> 16-bit rows: the one epilogue (the layer's later products run in enc_ffn16_kernel)

template <int PREC>
__device__ __forceinline__ void stage_rows16(const typename CT<PREC>::elem* a, size_t row0, size_t M, int K, int kc,
                                             typename CT<PREC>::elem* As, int tid) {
    const int piece = tid & 31;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = (tid >> 5) + 16 * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row0 + r < M) v = *reinterpret_cast<const uint4*>(a + (row0 + r) * K + kc * 256 + piece * 8);
        *reinterpret_cast<uint4*>(As + r * RS16 + piece * 8) = v;
    }
}

// acc (rows = this wave's 32 features, lane = token) + bias + residual h -> post-norm LayerNorm -> h (fp32, whole lines through
// the XOR-swizzled LDS transpose) and hx (16-bit, rows of the normalised tile as they lie in LDS).  `smem`: >= 128 KiB staging
// area starting at the tile As; P1 / P2 behind it.
template <int PREC>
__device__ __forceinline__ int res_ln(f32x16 (&acc)[4], const float* __restrict__ bias, const float* __restrict__ h,
                                      const float* ln_g, const float* ln_b, float eps, size_t row0, size_t M,
                                      typename CT<PREC>::elem* As, float* P1, float* P2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lhalf = lane >> 5;
    // r = acc + bias + residual (this lane's token, 4 consecutive features per quad)
    const float* bp = bias + wave * 32 + 4 * lhalf;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const size_t row = row0 + mt * 32 + lrow;
        const float* hr = (h ? h : bias) + (h && row < M ? row : 0) * D + wave * 32 + 4 * lhalf;   // h == nullptr: no residual here
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bb = *reinterpret_cast<const float4*>(bp + 8 * q);
            float4 hv = *reinterpret_cast<const float4*>(hr + 8 * q);
            if (!h) hv = make_float4(0.f, 0.f, 0.f, 0.f);
            acc[mt][4 * q + 0] += bb.x + hv.x;
            acc[mt][4 * q + 1] += bb.y + hv.y;
            acc[mt][4 * q + 2] += bb.z + hv.z;
            acc[mt][4 * q + 3] += bb.w + hv.w;
        }
    }
    const int l_valid = (int)std::min<size_t>(M > row0 ? M - row0 : 0, 128);
    ln_acc_to_tile<PREC, true>(acc, P1, P2, ln_g, ln_b, eps, As, 0, l_valid, wave, lrow, lhalf);
    return l_valid;
}

// the normalised tile (As, 16-bit) -> hx rows; the normalised accumulators -> h (fp32, whole 128-byte lines through the
// XOR-swizzled LDS transpose, which overwrites the first 128 KiB of `smem`, As included)
template <int PREC>
__device__ __forceinline__ void store_h_hx(const f32x16 (&acc)[4], float* __restrict__ h, typename CT<PREC>::elem* __restrict__ hx,
                                           size_t row0, int l_valid, unsigned char* smem, const typename CT<PREC>::elem* As) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    {
        const int piece = tid & 31;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = (tid >> 5) + 16 * i;
            if (r < l_valid)
                *reinterpret_cast<uint4*>(hx + (row0 + r) * D + piece * 8) = *reinterpret_cast<const uint4*>(As + r * RS16 + piece * 8);
        }
    }
    __syncthreads();
    float* rs = reinterpret_cast<float*>(smem) + wave * (128 * 32);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int tok = mt * 32 + lrow;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int chunk = (2 * q + lhalf) ^ (tok & 7);
            *reinterpret_cast<float4*>(rs + tok * 32 + 4 * chunk) =
                make_float4(acc[mt][4 * q + 0], acc[mt][4 * q + 1], acc[mt][4 * q + 2], acc[mt][4 * q + 3]);
        }
    }
    const int c = lane & 7, rsub = lane >> 3;
    float* hrow = h + row0 * D + wave * 32 + 4 * c;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int tr = i * 8 + rsub;
        const float4 v = *reinterpret_cast<const float4*>(rs + tr * 32 + 4 * (c ^ (tr & 7)));
        if (tr < l_valid) *reinterpret_cast<float4*>(hrow + (size_t)tr * D) = v;
    }
}

// N / 256 blocks of a bias (+ReLU) linear layer over the staged tile As, 16-bit token-major output through the wave-private
// tiles at `zs`.  On entry bs[0] holds the first half-set of block 0.
template <int PREC, int N>
__device__ __forceinline__ void act_blocks(const typename CT<PREC>::elem* As, typename CT<PREC>::elem* zs, const u16x8* wp,
                                           const float* __restrict__ bias, typename CT<PREC>::elem* out, size_t row0, size_t M,
                                           bool relu, u16x8 (&bs)[2][1][SETK], f32x16 (&acc)[4]) {
    using elem = typename CT<PREC>::elem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lhalf = lane >> 5;
#pragma unroll 1
    for (int nb = 0; nb < N / 256; ++nb) {
        zero_acc(acc);
        phase_tm<PREC, D, D, true>(As, wp, nb, 0, wp, nb + 1 < N / 256 ? nb + 1 : 0, 0, wave, lane, bs, acc);
        // rows = features (register quads), lane = token
        const float* bp = bias + nb * 256 + wave * 32 + 4 * lhalf;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bb = *reinterpret_cast<const float4*>(bp + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                float v0 = acc[mt][4 * q + 0] + bb.x, v1 = acc[mt][4 * q + 1] + bb.y, v2 = acc[mt][4 * q + 2] + bb.z,
                      v3 = acc[mt][4 * q + 3] + bb.w;
                if (relu) v0 = fmaxf(v0, 0.f), v1 = fmaxf(v1, 0.f), v2 = fmaxf(v2, 0.f), v3 = fmaxf(v3, 0.f);
                u16x4 pk = {to_bits<PREC>(v0), to_bits<PREC>(v1), to_bits<PREC>(v2), to_bits<PREC>(v3)};
                *reinterpret_cast<u16x4*>(zs + (mt * 32 + lrow) * ZRS + 8 * q + 4 * lhalf) = pk;
            }
        }
        const size_t valid = M > row0 ? M - row0 : 0;
        store_wave_tile<elem>(zs, out, row0, valid, N, nb * 256 + wave * 32, lane, 128);
    }
}

template <int PREC, int EPI, int K, int N>
__global__ __launch_bounds__(512) void linear16_kernel(LinArgs m) {
    using elem = typename CT<PREC>::elem;
    using frag = u16x8;
    static_assert(EPI == E_ACT && K == 256 && N % 256 == 0, "one activation tile, 256-wide output chunks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    elem* As = reinterpret_cast<elem*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * 128;
    const elem* a = reinterpret_cast<const elem*>(m.a);
    const frag* wp = reinterpret_cast<const frag*>(m.w);
    f32x16 acc[4];
    frag bs[2][1][SETK];
    elem* zs = As + 128 * RS16 + wave * 128 * ZRS;            // wave-private [128 tokens][32 features]
    load_set<PREC, K, 1>(wp, 0, 0, 0, wave, lane, bs[0]);
    __builtin_amdgcn_sched_barrier(0);
    stage_rows16<PREC>(a, row0, m.M, K, 0, As, tid);
    __syncthreads();
    act_blocks<PREC, N>(As, zs, wp, m.bias, reinterpret_cast<elem*>(m.out16), row0, m.M, m.relu != 0, bs, acc);
}

// ------------------------------------------------------------------------------------------------ fused feed-forward
// h = LN2(h + relu(hx W1^T + b1) W2^T + b2): the 1024-wide activations never reach HBM -- per 256-wide hidden chunk the fc1
// accumulator goes through bias + ReLU into an LDS tile that is the A operand of fc2's reduction chunk (same scheme as mlp16 in
// gemm16.hip); the post-norm LayerNorm runs on the fc2 accumulators and the new h / hx leave as whole lines.
struct FfnArgs {
    const void* hx_in;        // [M, 256] 16-bit
    const void *w1, *w2;      // packed [1024, 256], [256, 1024]
    const float *b1, *b2, *ln_g, *ln_b;
    float* h;                 // [M, 256] fp32, residual in / LayerNorm out
    void* hx_out;             // [M, 256] 16-bit copy of the new h (may alias hx_in: a tile is read completely before it is written)
    size_t M;
    float eps;
    const void* w_qkv;        // next layer's packed in_proj (null after the last layer): QKV of the tile just normalised
    const float* b_qkv;
    void* qkv;                // [M, 768] 16-bit
    // whole-layer form (att != null): the kernel starts from the attention output -- x1 = LN1(h + att W_o^T + b_o) stays in the
    // fc2 accumulators as the feed-forward residual and in LDS as its operand; h is read once and written once per layer
    const void* att;          // [M, 256] 16-bit; fp16c: two planes [2][M, 256] = fp16(64 a), fp16(64 a - hi) (attention.hip, HILO)
    const void* w_o;
    const float *b_o, *ln1_g, *ln1_b;
};

template <int PREC>
__global__ __launch_bounds__(512) void enc_ffn16_kernel(FfnArgs m) {
    using elem = typename CT<PREC>::elem;
    using frag = u16x8;
    constexpr int NCH = TFF / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    elem* As = reinterpret_cast<elem*>(smem);
    elem* Hs = As + 128 * RS16;
    float* P1 = reinterpret_cast<float*>(smem + (size_t)2 * 128 * RS16 * 2);
    float* P2 = P1 + 16 * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * 128;
    const frag* w1 = reinterpret_cast<const frag*>(m.w1);
    const frag* w2 = reinterpret_cast<const frag*>(m.w2);
    f32x16 acc1[4], acc2[4];
    frag bs[2][1][SETK];
    const bool whole = m.att != nullptr;                      // uniform
    if (whole) {
        const frag* wo = reinterpret_cast<const frag*>(m.w_o);
        load_set<PREC, D, 1>(wo, 0, 0, 0, wave, lane, bs[0]);
        load_set<PREC, D, 1>(wo, 0, 0, 1, wave, lane, bs[1]);
        __builtin_amdgcn_sched_barrier(0);
        stage_rows16<PREC>(reinterpret_cast<const elem*>(m.att), row0, m.M, D, 0, As, tid);
        if constexpr (PREC == PREC_F16C) stage_rows16<PREC>(reinterpret_cast<const elem*>(m.att) + m.M * D, row0, m.M, D, 0, Hs, tid);
        __syncthreads();
        zero_acc(acc2);
        if constexpr (PREC == PREC_F16C) {
            // out_proj of both planes of the attention output by the same weights, then the exact 1/64 of their common scale
            phase_tm<PREC, D, D, true, true>(As, wo, 0, 0, wo, 0, 0, wave, lane, bs, acc2);
            phase_tm<PREC, D, D, true>(Hs, wo, 0, 0, w1, 0, 0, wave, lane, bs, acc2);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[mt][r] *= 1.0f / 64.0f;
        } else {
            phase_tm<PREC, D, D, true, true>(As, wo, 0, 0, w1, 0, 0, wave, lane, bs, acc2);   // (the first fc1 set under its last set)
        }
        res_ln<PREC>(acc2, m.b_o, m.h, m.ln1_g, m.ln1_b, m.eps, row0, m.M, As, P1, P2);   // acc2 = x1, As = x1 (16-bit)
    } else {
        load_set<PREC, D, 1>(w1, 0, 0, 0, wave, lane, bs[0]);
        __builtin_amdgcn_sched_barrier(0);
        stage_rows16<PREC>(reinterpret_cast<const elem*>(m.hx_in), row0, m.M, D, 0, As, tid);
        __syncthreads();
        zero_acc(acc2);
    }
#pragma unroll 1
    for (int j = 0; j < NCH; ++j) {
        zero_acc(acc1);
        phase_tm<PREC, D, TFF, true>(As, w1, j, 0, w2, 0, j, wave, lane, bs, acc1);
        __syncthreads();                                       // every wave is done reading the previous chunk of Hs
        {
            const float* b1 = m.b1 + j * 256 + wave * 32 + 4 * lhalf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b1 + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    u16x4 pk = {to_bits<PREC>(fmaxf(acc1[mt][4 * q + 0] + bb.x, 0.f)), to_bits<PREC>(fmaxf(acc1[mt][4 * q + 1] + bb.y, 0.f)),
                                to_bits<PREC>(fmaxf(acc1[mt][4 * q + 2] + bb.z, 0.f)), to_bits<PREC>(fmaxf(acc1[mt][4 * q + 3] + bb.w, 0.f))};
                    *reinterpret_cast<u16x4*>(Hs + (mt * 32 + lrow) * RS16 + wave * 32 + 8 * q + 4 * lhalf) = pk;
                }
            }
        }
        __syncthreads();
        phase_tm<PREC, TFF, D, true>(Hs, w2, 0, j, w1, j + 1 < NCH ? j + 1 : 0, 0, wave, lane, bs, acc2);
    }
    if (m.w_qkv) load_set<PREC, D, 1>(reinterpret_cast<const frag*>(m.w_qkv), 0, 0, 0, wave, lane, bs[0]);
    const int l_valid = res_ln<PREC>(acc2, m.b2, whole ? nullptr : m.h, m.ln_g, m.ln_b, m.eps, row0, m.M, As, P1, P2);
    if (m.w_qkv) {   // in_proj of the next layer on the normalised tile while it is in LDS (wave tiles in the Hs + table region)
        elem* zs = Hs + wave * 128 * ZRS;
        act_blocks<PREC, TQKV>(As, zs, reinterpret_cast<const frag*>(m.w_qkv), m.b_qkv, reinterpret_cast<elem*>(m.qkv), row0, m.M,
                               false, bs, acc1);
    }
    store_h_hx<PREC>(acc2, m.h, reinterpret_cast<elem*>(m.hx_out), row0, l_valid, smem, As);
}

// ------------------------------------------------------------------------------------------------ pooling + classifier
// attn_weights = softmax_t(h[t] . w + b) over ALL positions of the read; pooled = sum_t a_t h[t]; Linear(256,128) ReLU Linear(128,2)
__global__ __launch_bounds__(256) void pool_head_kernel(const float* __restrict__ h, const float* __restrict__ pw,
                                                        const float* __restrict__ pb, const float* __restrict__ w0,
                                                        const float* __restrict__ b0, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, float* __restrict__ scores,
                                                        float* __restrict__ pooled_out, float* __restrict__ logits, int L3) {
    __shared__ float red[4], vec[4][D], xin[D], hid[TCH];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* hb = h + (size_t)b * L3 * D;
    float* sc = scores + (size_t)b * L3;
    const float4 w4 = *reinterpret_cast<const float4*>(pw + lane * 4);
    const float bias = pb[0];
    float mx = -INFINITY;
    for (int t = wave; t < L3; t += 4) {                      // one wave per position
        const float4 x = *reinterpret_cast<const float4*>(hb + (size_t)t * D + lane * 4);
        const float s = wave_sum((x.x * w4.x + x.y * w4.y) + (x.z * w4.z + x.w * w4.w)) + bias;
        if (lane == 0) sc[t] = s;
        mx = fmaxf(mx, s);
    }
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ssum = 0.f;
    for (int t = wave; t < L3; t += 4) {
        const float e = expf(sc[t] - mx);                     // written by lane 0 of this same wave above
        const float4 x = *reinterpret_cast<const float4*>(hb + (size_t)t * D + lane * 4);
        ssum += e;
        a0 = fmaf(e, x.x, a0); a1 = fmaf(e, x.y, a1); a2 = fmaf(e, x.z, a2); a3 = fmaf(e, x.w, a3);
    }
    *reinterpret_cast<float4*>(&vec[wave][lane * 4]) = make_float4(a0, a1, a2, a3);
    if (lane == 0) red[wave] = ssum;
    __syncthreads();
    {
        const float tot = (red[0] + red[1]) + (red[2] + red[3]);
        const float p = ((vec[0][tid] + vec[1][tid]) + (vec[2][tid] + vec[3][tid])) / tot;
        xin[tid] = p;
        pooled_out[(size_t)b * D + tid] = p;
    }
    __syncthreads();
    if (tid < TCH) {
        float acc = b0[tid];
        const float* wr = w0 + (size_t)tid * D;
        for (int i = 0; i < D; ++i) acc = fmaf(wr[i], xin[i], acc);
        hid[tid] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    if (tid < NCLS) {
        float acc = b1[tid];
        for (int i = 0; i < TCH; ++i) acc = fmaf(w1[(size_t)tid * TCH + i], hid[i], acc);
        logits[(size_t)b * NCLS + tid] = acc;
    }
}

}  // namespace tf

}  // namespace clm

// ================================================================================================ engine + C ABI
using namespace clm;

struct clm_tf_handle {
    int device = 0, prec = PREC_F16, n_layers = 12;
    std::string err;
    std::map<std::string, DevBuf> w;              // fp32 device copies by reference key
    WeightTable expected;                         // (clm_tf_create) every key but pos_encoder.pe, whose length is the tensor's own
    int max_len = 0;                              // positions of the loaded pos_encoder.pe [1, max_len, 256]
    // the weights resolved by clm_tf_finalize (pointers into `w`) and their packings, one per kind (a forward's choice: tf_run)
    std::vector<TfLayerF32> lay;                  // [n_layers], sized by clm_tf_create: `expected` points into it
    TfNetF32 net = {};
    TfPacking pk_mode;                            // the handle's 16-bit mode (none on an fp32 / fp16x3 handle)
    TfPacking pk_t32;                             // exact fp32: the fused kernels' packing (tail32.hip); a 16-bit handle's referee / fall-back
    TfPacking pk_x3;                              // the same weights as hi + lo halfs (have_x3)
    bool finalized = false;
    // workspace (tf_run)
    DevBuf ids8;
    DevBuf x1, x2, x3, hx, qkv, att;              // 16-bit activations
    DevBuf h, scores, pooled;                     // fp32; pooled [B][256] scales with B alone
    bool arith_x3 = false;                        // CLM_PREC_F16X3: prec is PREC_F32, the fused fp32-path kernels run on hi + lo halfs
    bool unfused_fp32 = false;                    // CLM_DEBUG=unfused_fp32 at creation: the separate fp32 launches of round 2 (tests cross-check the fused kernels)
    DevBuf ws32;                                  // fp32 mode: activations of tf_fp32.hip
    // How forwards run right now, read by plan_tf alone; clm_tf_selfcheck changes it for a scope (RunScope)
    struct RunMode {
        // clm_tf_set_fallback (as clm_set_fallback): 0 = the handle's mode; 1 = the next arithmetic inside the gate (16-bit handle: the
        // fp32-path kernels on hi + lo halfs = fp16x3; fp16x3 handle: exact fp32); 2 = exact fp32 (the raw fp32 tensors stay loaded)
        int fallback = 0;
        bool referee = false;                     // inside clm_tf_selfcheck's second pass: exact fp32, whatever the mode or fall-back level
        bool prof = false;                        // clm_tf_profile_enable: StageTimer records its spans
        // clm_tf_debug_stop_after (tests): a forward returns right after the launch of this CLM_TF_STAGE_* (< 0: the whole forward)
        int stop_after = -1;
    } run;
    // Everything a forward of B reads of L tokens decides, each decision once (plan_tf); `last`: the plan of the last forward, which
    // says what clm_tf_debug_fetch may hand out (B = 0: none yet)
    struct Plan {
        int B, L, L3, Lp;                         // L3 = L / 8 positions behind the stem, Lp = the row pitch of ids8
        size_t M, es;                             // M = B * L3 rows; bytes per element of the path's activations
        int prec;                                 // PREC_* of the kernels that run: the handle's 16-bit mode, or PREC_F32
        bool path32, x3, unfused;                 // the fp32-path kernels; ... on hi + lo halfs (fp16x3); ... as CLM_DEBUG=unfused_fp32's separate launches
        int stop;                                 // the CLM_TF_STAGE_* the forward ends behind (< 0: none)
    } last = {};
    bool have_x3 = false;                         // pk_x3 is filled (fp16x3 and 16-bit handles, fused kernels only)
    float x3_wmax = 0.f;                          // largest |w| they hold (NaN if any is NaN): from X3_WEIGHT_LIMIT on, exact fp32 instead
    DevBuf sc_logits;                             // clm_tf_selfcheck: [2][B][2] fp32 logits of the two forwards
    // profiling taps (clm_tf_profile_*): HIP events on the launch stream around each stage, stages: 0 conv stack + pe/LN,
    // 1 attention, 2 encoder layer kernel (out_proj + LN1 + FFN + LN2 + next QKV; the unfused pieces count here too), 3 pooling head
    StageProfile<4> profile;
};
using TfPlan = clm_tf_handle::Plan;

namespace {

// clm_tf_create: the state-dict keys of an n_layers-deep net, their shapes and the field of h->net / h->lay each resolves into
void tf_expect(clm_tf_handle* h) {
    WeightTable& e = h->expected;
    TfNetF32& n = h->net;
    h->lay.assign(h->n_layers, TfLayerF32{});
    e["embedding.weight"] = {{tf::TVOC, D}, &n.emb};
    for (int c = 0; c < 3; ++c) {
        e["cnn." + std::to_string(3 * c) + ".weight"] = {{D, D, 3}, &n.conv_w[c]};
        e["cnn." + std::to_string(3 * c) + ".bias"] = {{D}, &n.conv_b[c]};
    }
    e["norm.weight"] = {{D}, &n.norm_g}; e["norm.bias"] = {{D}, &n.norm_b};
    for (int i = 0; i < h->n_layers; ++i) {
        const std::string p = "transformer_encoder.layers." + std::to_string(i) + ".";
        TfLayerF32& l = h->lay[i];
        e[p + "self_attn.in_proj_weight"] = {{tf::TQKV, D}, &l.w[0]}; e[p + "self_attn.in_proj_bias"] = {{tf::TQKV}, &l.b_in};
        e[p + "self_attn.out_proj.weight"] = {{D, D}, &l.w[1]}; e[p + "self_attn.out_proj.bias"] = {{D}, &l.b_out};
        e[p + "linear1.weight"] = {{tf::TFF, D}, &l.w[2]}; e[p + "linear1.bias"] = {{tf::TFF}, &l.b_ff1};
        e[p + "linear2.weight"] = {{D, tf::TFF}, &l.w[3]}; e[p + "linear2.bias"] = {{D}, &l.b_ff2};
        e[p + "norm1.weight"] = {{D}, &l.ln1_g}; e[p + "norm1.bias"] = {{D}, &l.ln1_b};
        e[p + "norm2.weight"] = {{D}, &l.ln2_g}; e[p + "norm2.bias"] = {{D}, &l.ln2_b};
    }
    e["attn_pool.weight"] = {{1, D}, &n.pool_w}; e["attn_pool.bias"] = {{1}, &n.pool_b};
    e["classifier.0.weight"] = {{tf::TCH, D}, &n.cls0_w}; e["classifier.0.bias"] = {{tf::TCH}, &n.cls0_b};
    e["classifier.3.weight"] = {{NCLS, tf::TCH}, &n.cls3_w}; e["classifier.3.bias"] = {{NCLS}, &n.cls3_b};
}

void tf_pool_head(clm_tf_handle* h, int B, int L3, float* logits, hipStream_t st) {   // stage 3 of either path, on the residual stream h->h
    const TfNetF32& n = h->net;
    hipLaunchKernelGGL(tf::pool_head_kernel, dim3(B), dim3(256), 0, st, h->h.get<float>(), n.pool_w, n.pool_b, n.cls0_w, n.cls0_b, n.cls3_w,
                       n.cls3_b, h->scores.get<float>(), h->pooled.get<float>(), logits, L3);
}

// How a forward of B reads of L tokens runs on this handle right now: every decision once and under one name.  tf_run, the
// effective precision and (through h->last) the debug fetch read these fields; none looks at the handle's flags again.
TfPlan plan_tf(const clm_tf_handle* h, int B, int L) {
    TfPlan p{};
    const clm_tf_handle::RunMode& r = h->run;
    p.B = B; p.L = L; p.L3 = L / 8;
    p.Lp = (L + 63) / 64 * 64;
    p.M = (size_t)B * p.L3;
    // the fp32-path kernels: an fp32 / fp16x3 handle's own, a 16-bit handle's fall-back, the referee pass of a self-check
    p.path32 = h->prec == PREC_F32 || r.fallback > 0 || r.referee;
    // ... on hi + lo halfs: an fp16x3 handle unless told to fall back, a 16-bit handle at fall-back level 1.  Never as referee, and
    // exact fp32 instead where the weights are beyond the packing's range
    p.x3 = p.path32 && !r.referee && h->have_x3 && h->x3_wmax < X3_WEIGHT_LIMIT && (h->arith_x3 ? r.fallback == 0 : r.fallback < 2);
    p.unfused = p.path32 && h->unfused_fp32;
    p.prec = p.path32 ? (int)PREC_F32 : h->prec;
    p.es = p.path32 ? 4 : 2;
    p.stop = r.stop_after;
    return p;
}

// The launches of the handle's 16-bit mode.  false: the attention refused the shape and nothing behind it was launched; the launch
// error is the caller's to read.
template <int PREC>
bool tf_forward_t(clm_tf_handle* h, const TfPlan& p, const void* ids, int ids_dtype, int64_t stride, float* logits, hipStream_t st) {
    using elem = typename CT<PREC>::elem;
    const int B = p.B, L = p.L, L1 = L / 2, L2 = L1 / 2, L3 = p.L3, Lp = p.Lp;
    const size_t M = p.M;
    const TfNetF32& n = h->net;
    const TfPacking& pk = h->pk_mode;
    const int stop = p.stop;                                   // (< 0: never equal to a stage)
    {
        StageTimer t(h, st, 0);
        launch_embed(ids, ids_dtype, stride, nullptr, nullptr, h->ids8.get<unsigned char>(), B, L, Lp, st);   // ids of any dtype -> clamped uint8
        if (stop == CLM_TF_STAGE_EMBED) return true;          // (this path has no embedding launch: the first convolution reads the ids)
        constexpr size_t conv_lds = (size_t)(130 * RS16 + 8 * 64 * tf::ZRS) * 2;
        constexpr auto k1 = tf::conv3_relu_pool_kernel<PREC, true>;
        constexpr auto k2 = tf::conv3_relu_pool_kernel<PREC, false>;
        launch_lds<k1>(dim3((2 * L1 + 127) / 128, B), dim3(512), conv_lds, st, h->ids8.get<unsigned char>(), Lp, n.emb,
                       (const elem*)nullptr, pk.conv[0].get(), n.conv_b[0], h->x1.get<elem>(), L, L1);
        if (stop == CLM_TF_STAGE_CONV1) return true;
        launch_lds<k2>(dim3((2 * L2 + 127) / 128, B), dim3(512), conv_lds, st, (const unsigned char*)nullptr, 0,
                       (const float*)nullptr, h->x1.get<const elem>(), pk.conv[1].get(), n.conv_b[1], h->x2.get<elem>(), L1, L2);
        if (stop == CLM_TF_STAGE_CONV2) return true;
        launch_lds<k2>(dim3((2 * L3 + 127) / 128, B), dim3(512), conv_lds, st, (const unsigned char*)nullptr, 0,
                       (const float*)nullptr, h->x2.get<const elem>(), pk.conv[2].get(), n.conv_b[2], h->x3.get<elem>(), L2, L3);
        if (stop == CLM_TF_STAGE_CONV3) return true;
        hipLaunchKernelGGL(tf::pe_ln_kernel<PREC>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, h->x3.get<const elem>(), n.pe, n.norm_g,
                           n.norm_b, h->h.get<float>(), h->hx.get<elem>(), M, L3, 1e-5f);
        if (stop == CLM_TF_STAGE_PE_LN) return true;
    }
    for (int i = 0; i < h->n_layers; ++i) {
        const TfLayerF32& l = h->lay[i];
        const std::array<DevBuf, 4>& m = pk.mat[i];
        if (i == 0) {   // later layers: computed at the end of the previous layer's feed-forward kernel
            StageTimer t(h, st, 2);
            const tf::LinArgs a{h->hx.get(), m[0].get(), l.b_in, h->qkv.get(), M, 0};
            constexpr size_t lds = (size_t)(128 * RS16 + 8 * 128 * tf::ZRS) * 2;
            launch_lds<tf::linear16_kernel<PREC, tf::E_ACT, D, tf::TQKV>>(dim3((unsigned)((M + 127) / 128)), dim3(512), lds, st, a);
            if (stop == CLM_TF_STAGE_IN_PROJ) return true;
        }
        {
            StageTimer t(h, st, 1);
            if (!launch_attention_fwd(PREC, h->qkv.get(), h->att.get(), B, L3, st, PREC == PREC_F16C))   // fp16c: hi and lo planes (attention.hip)
                return false;
            if (stop == CLM_TF_STAGE_ATTENTION(i)) return true;
        }
        StageTimer tl(h, st, 2);
        // the rest of the layer -- out_proj + LN1 at its head -- and the next layer's in_proj: one kernel
        const bool more = i + 1 < h->n_layers;
        const tf::FfnArgs f{h->hx.get(), m[2].get(), m[3].get(), l.b_ff1, l.b_ff2, l.ln2_g, l.ln2_b, h->h.get<float>(), h->hx.get(), M, 1e-5f,
                            more ? pk.mat[i + 1][0].get() : nullptr, more ? h->lay[i + 1].b_in : nullptr, h->qkv.get(),
                            h->att.get(), m[1].get(), l.b_out, l.ln1_g, l.ln1_b};
        constexpr size_t lds = (size_t)2 * 128 * RS16 * 2 + (size_t)2 * 16 * 128 * 4;
        launch_lds<tf::enc_ffn16_kernel<PREC>>(dim3((unsigned)((M + 127) / 128)), dim3(512), lds, st, f);
        if (stop == CLM_TF_STAGE_LAYER(i)) return true;
    }
    {
        StageTimer t(h, st, 3);
        tf_pool_head(h, B, L3, logits, st);
    }
    return true;
}

}  // namespace

extern "C" {

int clm_tf_create(int device, int precision, int n_layers, clm_tf_handle** out) {
    if (!out || n_layers < 1 || n_layers > 64) return fail<clm_tf_handle>(nullptr, CLM_E_INVALID, "clm_tf_create: bad argument");
    if (precision != CLM_PREC_F16 && precision != CLM_PREC_BF16 && precision != CLM_PREC_F32 && precision != CLM_PREC_F16C &&
        precision != CLM_PREC_F16X3)
        return fail<clm_tf_handle>(nullptr, CLM_E_UNSUPPORTED,
                       "clm_tf_create: precision must be fp32 (exact, the reference's arithmetic), fp16x3, fp16c, fp16 or bf16");
    if (int rc = use_gfx950<clm_tf_handle>(device, "clm_tf_create")) return rc;
    clm_tf_handle* h = new clm_tf_handle();
    h->unfused_fp32 = debug_flag("unfused_fp32");
    h->device = device;
    // fp16x3: the exact-fp32 path with its fused kernels multiplying hi + lo halfs (three fp16 MFMAs per product; tail32.hip AR_X3)
    h->arith_x3 = precision == CLM_PREC_F16X3;
    if (h->arith_x3 && h->unfused_fp32) {
        delete h;
        return fail<clm_tf_handle>(nullptr, CLM_E_UNSUPPORTED, "clm_tf_create: fp16x3 exists in the fused kernels only (CLM_DEBUG=unfused_fp32 is set)");
    }
    h->prec = precision == CLM_PREC_BF16 ? PREC_BF16 : (precision == CLM_PREC_F32 || h->arith_x3) ? PREC_F32 : precision == CLM_PREC_F16C ? PREC_F16C
                                                                                                                                   : PREC_F16;
    h->n_layers = n_layers;
    tf_expect(h);
    *out = h;
    return CLM_OK;
}

int clm_tf_load_weight(clm_tf_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !key || !data || !shape) return fail(h, CLM_E_INVALID, "clm_tf_load_weight: null argument");
    if (dtype != CLM_DT_F32) return fail(h, CLM_E_INVALID, "clm_tf_load_weight: fp32 tensors only");
    const std::string k = canonical_weight_key(key);
    if (k != "pos_encoder.pe") return load_f32(h, "clm_tf_load_weight", k, data, shape, ndim);
    if (ndim != 3 || shape[0] != 1 || shape[2] != D) return fail(h, CLM_E_INVALID, "pos_encoder.pe: expected [1, max_len, 256]");   // a buffer
    if (int rc = store_f32(h, k, data, (size_t)shape[1] * D)) return rc;
    h->max_len = (int)shape[1];
    return CLM_OK;
}

int clm_tf_finalize(clm_tf_handle* h) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = resolve_weights(h, "clm_tf_finalize")) return rc;
    const auto pe = h->w.find("pos_encoder.pe");
    if (pe == h->w.end()) return fail(h, CLM_E_MISSING, "clm_tf_finalize: missing buffer pos_encoder.pe");
    h->net.pe = pe->second.get<float>();
    constexpr int MAT_N[4] = {tf::TQKV, D, tf::TFF, D}, MAT_K[4] = {D, D, D, tf::TFF};
    h->have_x3 = (h->arith_x3 || h->prec != PREC_F32) && !h->unfused_fp32;
    h->x3_wmax = 0.f;
    if (h->have_x3) {             // what the hi + lo packing must hold: the CNN stem and the four dense products of every layer
        auto track = [&](const float* w, size_t n) {
            float m = 0.f;
            const hipError_t e = device_max_abs(w, n, m);
            if (m != m || m > h->x3_wmax) h->x3_wmax = m;          // (NaN stays)
            return e;
        };
        for (const float* w : h->net.conv_w) HIPCHK(h, track(w, (size_t)3 * D * D));
        for (const TfLayerF32& l : h->lay)
            for (int j = 0; j < 4; ++j) HIPCHK(h, track(l.w[j], (size_t)MAT_N[j] * MAT_K[j]));
    }
    // Three kinds of packing.  t32: exact fp32 (the handle's own mode, or the referee / fall-back of a 16-bit handle), the dense layers
    // and the stem in the fused kernels' packing (tail32.hip); everything else of tf_fp32.hip reads the fp32 tensors as they are.
    // x3: the same as hi + lo halfs (an fp16x3 handle's mode, or a 16-bit handle's first fall-back level).  mode: a 16-bit handle's own.
    TfPacking* const pks[3] = {&h->pk_t32, &h->pk_x3, &h->pk_mode};
    const bool on[3] = {true, h->have_x3, h->prec != PREC_F32};
    auto bytes = [&](int q, int n, int k) { return q < 2 ? (size_t)n * k * 4 : packed_weight_bytes(h->prec, n, k); };
    auto pack = [&](int q, const float* src, void* out, int n, int k) {
        if (q == 0) launch_pack_f32t(src, out, n, k, 0);
        else if (q == 1) launch_pack_x3(src, out, n, k, 0);
        else launch_pack_weight(h->prec, src, out, n, k, 0);
    };
    for (TfPacking* pk : pks) *pk = TfPacking{};                   // (a reload leaves nothing of the packings before it)
    h->finalized = false;
    DevBuf split;                 // a stem convolution's three taps: [co][ci][3] -> [3][co][ci]
    HIPCHK(h, split.alloc((size_t)3 * D * D * 4));
    for (int q = 0; q < 3; ++q) {
        if (!on[q]) continue;
        pks[q]->mat.resize(h->n_layers);
        for (int i = 0; i < h->n_layers; ++i)
            for (int j = 0; j < 4; ++j) {
                HIPCHK(h, pks[q]->mat[i][j].alloc(bytes(q, MAT_N[j], MAT_K[j])));
                pack(q, h->lay[i].w[j], pks[q]->mat[i][j].get(), MAT_N[j], MAT_K[j]);
            }
        for (int c = 0; c < 3; ++c) {   // (pack_taps synchronises: `split` is reused by the next convolution, and freed after the last)
            hipLaunchKernelGGL(tf::conv_w_split_kernel, dim3((3 * D * D + 255) / 256), dim3(256), 0, 0, h->net.conv_w[c], split.get<float>());
            auto tap = [&](const float* src, void* out) { pack(q, src, out, D, D); };
            if (int rc = pack_taps(h, split.get<float>(), 3, bytes(q, D, D), pks[q]->conv[c], tap)) return rc;
        }
    }
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    return CLM_OK;
}

// One forward as `p` plans it (workspaces of BOTH paths may be live on one handle: the self-check runs one after the other on the
// same ids).  Every buffer the path takes grows on its own: a handle holds the per-buffer maxima of the shapes it has seen.
static int tf_run(clm_tf_handle* h, const TfPlan& p, const void* ids, int ids_dtype, int64_t ids_row_stride, float* logits_out, hipStream_t st) {
    const size_t B = (size_t)p.B, L = (size_t)p.L, M = p.M;
    const size_t e16 = p.path32 ? 0 : 2;                       // the 16-bit activations: none on the fp32 path
    if (int rc = grow(h, Sync::Device(), {{&h->ids8, B * p.Lp}, {&h->h, M * D * 4}, {&h->scores, M * 4}, {&h->pooled, B * D * 4},
                                          {&h->ws32, p.path32 ? tf32_workspace_floats(p.B, p.L) * 4 : 0},
                                          {&h->x1, B * (L / 2) * D * e16}, {&h->x2, B * (L / 4) * D * e16}, {&h->x3, M * D * e16},
                                          {&h->hx, M * D * e16}, {&h->qkv, M * tf::TQKV * e16},
                                          {&h->att, M * D * e16 * (p.prec == PREC_F16C ? 2 : 1) /* hi + lo planes */}}))
        return rc;
    bool ran;
    if (p.path32) {
        launch_embed(ids, ids_dtype, ids_row_stride, nullptr, nullptr, h->ids8.get<unsigned char>(), p.B, p.L, p.Lp, st);
        ran = tf32_forward(h->ids8.get<unsigned char>(), p.Lp, p.B, p.L, h->n_layers, h->ws32.get<float>(), h->h.get<float>(), h->net,
                           h->lay.data(), p.x3 ? h->pk_x3 : h->pk_t32, st, p.unfused, p.x3, p.stop);
        if (ran && p.stop < 0) tf_pool_head(h, p.B, p.L3, logits_out, st);   // (stopped: nothing behind that launch, the pooling head included)
    } else {
        ran = p.prec == PREC_BF16   ? tf_forward_t<PREC_BF16>(h, p, ids, ids_dtype, ids_row_stride, logits_out, st)
              : p.prec == PREC_F16C ? tf_forward_t<PREC_F16C>(h, p, ids, ids_dtype, ids_row_stride, logits_out, st)
                                    : tf_forward_t<PREC_F16>(h, p, ids, ids_dtype, ids_row_stride, logits_out, st);
    }
    if (!ran)
        return fail(h, CLM_E_INVALID, "clm_tf_forward: the attention refused " + std::to_string(p.B) + " reads of " + std::to_string(p.L3) +
                                          " positions: more workgroups than a grid takes");
    if (int rc = launched(h, p.path32 ? "clm_tf_forward (fp32)" : "clm_tf_forward")) return rc;
    h->last = p;                                               // what clm_tf_debug_fetch may hand out after this forward
    return CLM_OK;
}

static int tf_check_args(clm_tf_handle* h, const char* who, const void* ids, const void* out, int ids_dtype, int64_t ids_row_stride, int B, int L) {
    if (!h->finalized) return fail(h, CLM_E_STATE, std::string(who) + " before clm_tf_finalize");
    if (int rc = check_ids_arg(h, who, ids, out, ids_dtype, ids_row_stride, B, L, 8)) return rc;   // (three max-pools of 2)
    if (L / 8 > h->max_len)
        return fail(h, CLM_E_INVALID, std::string(who) + ": Sequence too long (" + std::to_string(L / 8) + " > max_len of pos_encoder.pe)");
    return CLM_OK;
}

int clm_tf_forward(clm_tf_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                   void* stream) {
    if (!h) return CLM_E_INVALID;
    if (int rc = tf_check_args(h, "clm_tf_forward", ids, logits_out, ids_dtype, ids_row_stride, B, L)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return tf_run(h, plan_tf(h, B, L), ids, ids_dtype, ids_row_stride, logits_out, reinterpret_cast<hipStream_t>(stream));
}

// The handle's 16-bit mode on trial against the exact-fp32 kernels of the same handle, on the caller's ids (chimeralm_hip.h;
// the counterpart of clm_selfcheck).  Synchronises `stream`.
int clm_tf_selfcheck(clm_tf_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, void* stream,
                     float* max_abs_diff_out, int* labels_differ_out) {
    if (!h) return CLM_E_INVALID;
    if (int rc = tf_check_args(h, "clm_tf_selfcheck", ids, h, ids_dtype, ids_row_stride, B, L)) return rc;   // (both outputs are optional)
    if (B > 4096) return fail(h, CLM_E_INVALID, "clm_tf_selfcheck: at most 4096 reads per call");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float diff = 0.f;
    int differ = 0;
    if (h->prec != PREC_F32 || h->arith_x3) {                  // (an fp16x3 handle: its own exact-fp32 kernels are the referee)
        if (int rc = grow(h, Sync::Device(), {{&h->sc_logits, (size_t)2 * B * NCLS * 4}})) return rc;
        float* const pair = h->sc_logits.get<float>();
        {
            RunScope<clm_tf_handle> scope(h);
            h->run.fallback = 0;                               // the MODE is on trial, whatever clm_tf_set_fallback says
            h->run.stop_after = -1;                            // ... on whole forwards, whatever clm_tf_debug_stop_after says
            for (int pass = 0; pass < 2; ++pass) {             // pass 0: the handle's mode; pass 1: exact fp32
                h->run.referee = pass == 1;
                if (int rc = tf_run(h, plan_tf(h, B, L), ids, ids_dtype, ids_row_stride, pair + (size_t)pass * B * NCLS, st)) return rc;
            }
        }
        if (int rc = logits_deviation(h, st, pair, B, &diff, &differ)) return rc;
    }
    if (max_abs_diff_out) *max_abs_diff_out = diff;
    if (labels_differ_out) *labels_differ_out = differ;
    return CLM_OK;
}

int clm_tf_set_fallback(clm_tf_handle* h, int on) {
    if (!h) return CLM_E_INVALID;
    if (on < 0 || on > 2) return fail(h, CLM_E_INVALID, "clm_tf_set_fallback: level must be 0, 1 or 2");
    h->run.fallback = (h->prec == PREC_F32 && !h->arith_x3) ? 0 : on;
    return CLM_OK;
}

int clm_tf_effective_precision(const clm_tf_handle* h) {
    if (!h) return CLM_E_INVALID;
    if (!h->finalized) return CLM_E_STATE;
    const TfPlan p = plan_tf(h, 1, 8);                         // (the arithmetic does not depend on the shape)
    return p.x3 ? CLM_PREC_F16X3 : p.prec;
}

int clm_tf_debug_fetch(clm_tf_handle* h, const char* name, void* host_out, size_t bytes) {
    if (!h || !name || !host_out) return fail(h, CLM_E_INVALID, "clm_tf_debug_fetch: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const std::string n(name);
    const TfPlan& p = h->last;                                 // the last forward: its shape, its path, where it stopped
    const size_t B = (size_t)p.B, M = p.M, es = p.es;
    const int L = p.L, s = p.stop;
    const bool p32 = p.path32;
    const bool fused32 = p32 && !p.unfused;                    // the exact path's names below describe the fused launches' workspace
    auto ran = [&](int stage) { return p.B > 0 && (s < 0 || s >= stage); };   // the last forward launched `stage`
    const void* src = nullptr;
    size_t have = 0;
    bool produced = true;
    if (n == "hidden") { src = h->h.get(); have = M * D * 4; produced = ran(CLM_TF_STAGE_PE_LN); }
    else if (n == "scores") { src = h->scores.get(); have = M * 4; produced = p.B > 0 && s < 0; }
    else if (n == "pooled") { src = h->pooled.get(); have = B * D * 4; produced = p.B > 0 && s < 0; }
    else if (n == "x0") {       // exact path: the embedding rows, gone once the second convolution has written over them
        src = h->ws32.get(); have = B * L * D * 4; produced = fused32 && (s == CLM_TF_STAGE_EMBED || s == CLM_TF_STAGE_CONV1);
    } else if (n == "x1") {     // exact path: the other half of the ping-pong, until the third convolution
        src = p32 ? (const void*)(h->ws32.get<float>() + B * L * D) : h->x1.get(); have = B * (L / 2) * D * es;
        produced = p32 ? fused32 && (s == CLM_TF_STAGE_CONV1 || s == CLM_TF_STAGE_CONV2) : ran(CLM_TF_STAGE_CONV1);
    } else if (n == "x2") {
        src = p32 ? h->ws32.get() : h->x2.get(); have = B * (L / 4) * D * es; produced = (fused32 || !p32) && ran(CLM_TF_STAGE_CONV2);
    } else if (n == "x3") {
        src = p32 ? (const void*)(h->ws32.get<float>() + B * L * D) : h->x3.get(); have = M * D * es; produced = (fused32 || !p32) && ran(CLM_TF_STAGE_CONV3);
    } else if (n == "hx") { src = h->hx.get(); have = M * D * 2; produced = !p32 && ran(CLM_TF_STAGE_PE_LN); }
    else if (n == "qkv") {
        src = p32 ? (const void*)(h->ws32.get<float>() + (size_t)2 * B * L * D) : h->qkv.get(); have = M * tf::TQKV * es;
        produced = (fused32 || !p32) && ran(CLM_TF_STAGE_IN_PROJ);
    } else if (n == "att") {    // fp16c: both planes
        src = p32 ? (const void*)(h->ws32.get<float>() + (size_t)2 * B * L * D + M * tf::TQKV) : h->att.get();
        have = M * D * es * (p.prec == PREC_F16C ? 2 : 1); produced = (fused32 || !p32) && ran(CLM_TF_STAGE_ATTENTION(0));
    } else return fail(h, CLM_E_INVALID, "clm_tf_debug_fetch: unknown name " + n);
    if (!produced) return fail(h, CLM_E_INVALID, "clm_tf_debug_fetch: the last forward did not produce (or has overwritten) " + n);
    return fetch_bytes(h, "clm_tf_debug_fetch", n, src, have, host_out, bytes);
}

int clm_tf_debug_stop_after(clm_tf_handle* h, int stage) {
    if (!h) return CLM_E_INVALID;
    if (stage >= 0 && h->unfused_fp32) return fail(h, CLM_E_UNSUPPORTED, "clm_tf_debug_stop_after: the fused launches only (CLM_DEBUG=unfused_fp32 is set)");
    if (stage > CLM_TF_STAGE_LAYER(h->n_layers - 1)) return fail(h, CLM_E_INVALID, "clm_tf_debug_stop_after: no such stage in this net");
    h->run.stop_after = stage < 0 ? -1 : stage;
    return CLM_OK;
}

int clm_tf_profile_enable(clm_tf_handle* h, int on) {
    if (!h) return CLM_E_INVALID;
    h->run.prof = on != 0;
    return CLM_OK;
}

int clm_tf_profile_read(clm_tf_handle* h, double* ms_out /*[4]*/, int64_t* spans_out /*[4]*/, int reset) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    h->profile.read(ms_out, spans_out, reset != 0);
    return CLM_OK;
}

const char* clm_tf_last_error(const clm_tf_handle* h) { return h ? h->err.c_str() : create_error<clm_tf_handle>().c_str(); }

int clm_tf_destroy(clm_tf_handle* h) { return destroy_handle(h); }

}  // extern "C"
