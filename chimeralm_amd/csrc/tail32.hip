// tail32.hip -- the fused kernels of the exact-fp32 engine and of its fp16x3 form (round 4):
//   tail32_kernel   Hyena block tail (this comment)                          enc32_kernel   SequenceCNNTransformer encoder layer
//   conv32_kernel   the transformer's CNN stem (conv k = 3 + ReLU + pool)     pack_f32t / pack_x3 kernels: the weight packings
//   cnn_gemm7_kernel  DNAConvNet blocks 1 and 2 (conv k = 7 + BatchNorm + GELU + pool of 4; cnn.hip)
// all on one 64-token tile, one weight-set pipeline and one MFMA loop, instantiated for two arithmetics (AR_F32: the fp32 MFMA;
// AR_X3: every operand as two halfs, three fp16 MFMAs per product -- see ARITH below).  The fp32 / x3 attention lives in tf_fp32.hip.
//
// One kernel per Hyena block, on v_mfma_f32_32x32x2_f32 throughout, for the part of the block that is token-wise
//   /root/reference/chimeralm/models/components/hyena.py:244-256 -> the backbone's block: x = x + mixer(norm1(x)); x = x + mlp(norm2(x))
//       r  = h + b_out + W_out y                    (y = the convolution's output, channel-major in HBM)
//       h' = r + b_2 + W_2 gelu_tanh(W_1 LN2(r) + b_1)
//       z  = W_in' LN1'(h') + b_in'                 (the NEXT block's in_proj, rows x0 | x1 | v as the fp32 convolution reads them)
// where round 1-3's fp32 path ran five separate GEMM kernels per block with the 1024-wide fc1 output, the normalised tiles and
// the intermediate residual all crossing HBM in fp32 (gemm.hip; kept: block 0's in_proj, the score layer, and the whole path
// under CLM_DEBUG=unfused_fp32, which tests/ uses to cross-check this kernel).
//
// Tile = 64 tokens x 256 features per workgroup (8 waves; a wave owns 32 output features of every product, both 32-token row
// tiles): an fp32 tile of 64 tokens fills the LDS a 16-bit tile of 128 does (As + Hs = 2 x 65 KiB).  Weights are the MFMA's A
// operand (accumulator rows = output features, lane = token), packed per (256-wide block, wave, 8-deep k-step, lane) as one
// float4 -- the four k values a lane feeds to four consecutive MFMAs: the reduction index may be permuted freely, so MFMA j of a
// k-step pairs k = 8 s + j (lanes 0-31) with k = 8 s + 4 + j (lanes 32-63) and both operands are 16-byte loads.  A 64-deep weight
// set (8 float4 = 32 registers) is requested one set ahead of its use; a set is 64 MFMAs of 64 cycles per wave, so neither the
// L2 latency nor the 16 ds_read_b128 of a set are anywhere near the matrix pipe's time: the kernel is MFMA-bound by construction
// (12 blocks x 256 MFMAs x 64 cycles x 2 waves per SIMD = 393k cycles per tile against ~25k of LayerNorm / GELU / epilogue VALU).
#include "chimeralm_hip.h"
#include "clm_common.h"
#include "cnn_common.h"

#include "mfma32_common.h"

namespace clm {

struct Tail32Args {
    const float* y;           // [B, 256, Lp] fp32
    float* h;                 // [B, L, 256] residual stream, updated in place
    const f32x4 *w_out, *w_fc1, *w_fc2, *w_in;   // packed (pack_f32t_kernel); w_in: the NEXT block's in_proj
    const float *b_out, *b_fc1, *b_fc2, *b_in, *ln2_g, *ln2_b, *n_g, *n_b;
    float* z;                 // [B, 768, Lp] fp32 (NEXT)
    int B, L, Lp, tiles_x;
    float eps;
    const int* p0;            // [B] or null: 128-token tiles wholly inside each read's [PAD] prefix (pad_prefix.hip) -- not computed
    // NEXT = T32_SCORE (the last block): w_in = attention.0.weight (packed like the others), b_in = its bias, n_g / n_b = ln_f
    const float *att_w2, *att_b2;   // attention.2 weight [256] and bias [1]
    float* scores;            // [B, L] pooling scores
    float* partial;           // [B, tiles_x, POOL_PSTRIDE] per-tile online-softmax pooling partials (64-token tiles here)
    // block 0 with the id-table convolution: the residual entering the block is the embedding row of the token id -- gathered here,
    // the embedding kernel's 1 KiB per token never crosses HBM (as in the 16-bit tail kernel)
    const unsigned char* ids8;   // [B, Lp] or null
    const float* emb;            // [16, 256]
};

// NEXT: what follows the block on the tile still in registers -- the next block's LayerNorm-1 + in_proj / (round 5, the
// last block) ln_f + attention.0 + GELU(erf) + attention.2 = the pooling scores and this tile's online-softmax pooling partial, as
// the 16-bit tail kernel has it (gemm16.hip score_pool_tile; /root/reference/chimeralm/models/components/hyena.py:117-132): the
// separate score GEMM (3.5 ms per 256 x 8,193 launch), softmax-statistics and pooling kernels of rounds 1-4 read the fp32 residual
// stream twice more; head_tiles_kernel (head.hip) merges the partials in a fixed order.
enum { T32_INPROJ = 1, T32_SCORE = 2 };

template <int NEXT, int AR = AR_F32>
__global__ __launch_bounds__(512) void tail32_kernel(Tail32Args m) {
    constexpr float WSI = WUNSCALE<AR>;
    extern __shared__ __attribute__((aligned(16))) float smem32[];
    float* As = smem32;                                     // LN2(r) / LN1'(h') tile [64][RS32]      (the y tile aliases As + Hs)
    float* Hs = As + BM32 * RS32;                           // gelu(fc1) chunk [64][RS32]
    float* Ys = smem32;                                     // y tile [256 channels][RSY], k-major
    float* P1 = smem32 + 2 * BM32 * RS32;                   // LayerNorm partials [8][64]
    float* P2 = P1 + 8 * BM32;
    static_assert(D * RSY <= 2 * BM32 * RS32 && 2 * D * RSKM64 * 2 <= 2 * BM32 * RS32 * 4, "the y tile fits As + Hs");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int b = (int)blockIdx.x / m.tiles_x, t0 = ((int)blockIdx.x % m.tiles_x) * BM32, L = m.L, Lp = m.Lp;
    // a tile wholly inside the read's [PAD] prefix: its rows of z (and of the final h) come from the all-[PAD] table, nothing here
    // reads its neighbours (raw in_proj rows: the short filter runs in the convolution)  -- whole workgroup, before any barrier
    if (m.p0 && t0 + BM32 <= 128 * m.p0[b]) return;
    const int valid = L - t0 < BM32 ? L - t0 : BM32;
    f32x4 ws[2][KS_SET];
    f32x16 acc1[2], acc2[2];
    load_wset(wset_ptr(m.w_out, 0, D / 8, 0, wave, lane), ws[0]);
    // ---- 0. y tile -> LDS (k-major, as it lies in HBM): 16 lanes x 16 bytes per channel row, 32 channels per pass
    {
        const int tk = (tid & 15) * 4;
        const float* src = m.y + (size_t)b * D * Lp + t0 + tk;
        const bool in_row = t0 + tk < Lp;                   // (Lp is a multiple of 64: a 16-byte piece is inside the row or beyond it)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (tid >> 4) + 32 * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (in_row) v = *reinterpret_cast<const f32x4*>(src + (size_t)c * Lp);
            if constexpr (AR == AR_X3) {                    // two planes of halfs [channel][RSKM64]
                h4_t hi, lo;
                split4(v, hi, lo);
                _Float16* yh = reinterpret_cast<_Float16*>(Ys) + c * RSKM64 + tk;
                *reinterpret_cast<h4_t*>(yh) = hi;
                *reinterpret_cast<h4_t*>(yh + D * RSKM64) = lo;
            } else {
                *reinterpret_cast<f32x4*>(Ys + c * RSY + tk) = v;
            }
        }
    }
    // ---- 1. r = h + b_out + W_out y.  The products are summed from zero and the residual row joins the finished sum: with the
    //         residual in the accumulator from the start (rounds 4-5) every one of the 128 + 512 MFMA steps of out_proj and fc2
    //         rounded at the RESIDUAL's magnitude, not the sum's -- ~2.5e-6 of a row's largest value per token and block tail
    //         whatever the read length, ten times the reference's own fp32 error at the first tokens of a read
    //         (tests/test_gpu_per_token.py: 1 and 2 tokens).  `res` holds the residual next to the accumulators: 32 registers more,
    //         of the 256 a wave has at the two waves per SIMD that the LDS tiles allow anyway
    f32x16 res[2];
    {
        const float* bo = m.b_out + wave * 32 + 4 * lhalf;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int t = t0 + mt * 32 + lrow, tc = t < L ? t : L - 1;
            const float* row = m.ids8 ? m.emb + (size_t)m.ids8[(size_t)b * Lp + tc] * D + wave * 32 + 4 * lhalf
                                      : m.h + ((size_t)b * L + tc) * D + wave * 32 + 4 * lhalf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 hv = *reinterpret_cast<const float4*>(row + 8 * q);
                const float4 bb = *reinterpret_cast<const float4*>(bo + 8 * q);
                res[mt][4 * q + 0] = hv.x + bb.x;
                res[mt][4 * q + 1] = hv.y + bb.y;
                res[mt][4 * q + 2] = hv.z + bb.z;
                res[mt][4 * q + 3] = hv.w + bb.w;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[mt][r] = 0.f;
        }
    }
    __syncthreads();
    product256<true, AR>(Ys, m.w_out, 0, D / 8, 0, wset_ptr(m.w_fc1, 0, D / 8, 0, wave, lane), wave, lane, ws, acc2);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[mt][r] = acc2[mt][r] * WSI + res[mt][r];
    // ---- 2. LayerNorm-2 -> As; r moves to `res`, the accumulators take fc2's sum from zero
    ln_to_tile<false, AR>(acc2, P1, P2, m.ln2_g, m.ln2_b, m.eps, As, valid, wave, lrow, lhalf);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            res[mt][r] = acc2[mt][r];
            acc2[mt][r] = 0.f;
        }
    // ---- 3. MLP in four 256-wide chunks of the hidden layer (acc2: fc2's sum)
#pragma unroll 1
    for (int j = 0; j < DI / 256; ++j) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[mt][r] = 0.f;
        product256<false, AR>(As, m.w_fc1, j, D / 8, 0, wset_ptr(m.w_fc2, 0, DI / 8, j * 32, wave, lane), wave, lane, ws, acc1);
        {
            const float* b1 = m.b_fc1 + j * 256 + wave * 32 + 4 * lhalf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b1 + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    f32x4 g = {gelu_tanh(acc1[mt][4 * q + 0] * WSI + bb.x), gelu_tanh(acc1[mt][4 * q + 1] * WSI + bb.y),
                               gelu_tanh(acc1[mt][4 * q + 2] * WSI + bb.z), gelu_tanh(acc1[mt][4 * q + 3] * WSI + bb.w)};
                    tile_store4<AR>(Hs, mt * 32 + lrow, wave * 32 + 8 * q + 4 * lhalf, g);
                }
            }
        }
        __syncthreads();
        const f32x4* nxt = j + 1 < DI / 256 ? wset_ptr(m.w_fc1, j + 1, D / 8, 0, wave, lane)
                                            : wset_ptr(m.w_in, 0, D / 8, 0, wave, lane);
        product256<false, AR>(Hs, m.w_fc2, 0, DI / 8, j * 32, nxt, wave, lane, ws, acc2);
        __syncthreads();                                    // every wave is done reading Hs before the next chunk lands in it
    }
    // ---- 4. h' = r + acc2 + b_2: 16 bytes per lane and feature quad (a lane = a token row of h)
    {
        const float* b2p = m.b_fc2 + wave * 32 + 4 * lhalf;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bb = *reinterpret_cast<const float4*>(b2p + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                acc2[mt][4 * q + 0] = (acc2[mt][4 * q + 0] * WSI + bb.x) + res[mt][4 * q + 0];
                acc2[mt][4 * q + 1] = (acc2[mt][4 * q + 1] * WSI + bb.y) + res[mt][4 * q + 1];
                acc2[mt][4 * q + 2] = (acc2[mt][4 * q + 2] * WSI + bb.z) + res[mt][4 * q + 2];
                acc2[mt][4 * q + 3] = (acc2[mt][4 * q + 3] * WSI + bb.w) + res[mt][4 * q + 3];
                if (mt * 32 + lrow < valid)
                    *reinterpret_cast<float4*>(m.h + ((size_t)b * L + t0 + mt * 32 + lrow) * D + wave * 32 + 4 * lhalf + 8 * q) =
                        make_float4(acc2[mt][4 * q + 0], acc2[mt][4 * q + 1], acc2[mt][4 * q + 2], acc2[mt][4 * q + 3]);
            }
        }
    }
    // ---- 5. the next block's LayerNorm-1 (the last block: ln_f) -> As, and on the tile still in registers: in_proj, z rows x0 | x1 | v
    ln_to_tile<false, AR>(acc2, P1, P2, m.n_g, m.n_b, m.eps, As, valid, wave, lrow, lhalf);
    if constexpr (NEXT == T32_INPROJ) {
#pragma unroll 1
        for (int nb = 0; nb < D3 / 256; ++nb) {
            zero_acc(acc1);
            product256<false, AR>(As, m.w_in, nb, D / 8, 0, wset_ptr(m.w_in, nb + 1 < D3 / 256 ? nb + 1 : 0, D / 8, 0, wave, lane), wave,
                                  lane, ws, acc1);
            // rows = features: 32 lanes = 32 consecutive tokens of one channel row (128 bytes)
            const float* bi = m.b_in + nb * 256 + wave * 32 + 4 * lhalf;
            float* zb = m.z + ((size_t)b * D3 + nb * 256 + wave * 32 + 4 * lhalf) * Lp + t0 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = acc_row(r, 0);
                const float bias = bi[f];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    if (mt * 32 + lrow < valid) zb[(size_t)f * Lp + mt * 32] = acc1[mt][r] * WSI + bias;
            }
        }
    }
    // ---- 5'. the last block: scores, and this tile's pooling partial  m = max s_t, S = sum exp(s_t - m),
    //          vec[c] = sum_t exp(s_t - m) ln_f(h')[t][c]   (softmax over ALL positions, pads included: hyena.py:121-132, mask None)
    if constexpr (NEXT == T32_SCORE) {
        zero_acc(acc1);
        product256<false, AR>(As, m.w_in, 0, D / 8, 0, wset_ptr(m.w_in, 0, D / 8, 0, wave, lane), wave, lane, ws, acc1);   // (last slot: unused re-request)
        float* P = Hs;                                      // [8][64] score partials of the waves (Hs is dead: every wave is past the MLP)
        float* E = P + 8 * BM32;                            // [64] exp(s - m)
        float* V = E + BM32;                                // [4][256] pooled-vector partials of the four 16-token groups
        {
            const float* b1 = m.b_in + wave * 32 + 4 * lhalf;
            const float* w2 = m.att_w2 + wave * 32 + 4 * lhalf;
            float sc[2] = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b1 + 8 * q), ww = *reinterpret_cast<const float4*>(w2 + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    sc[mt] = fmaf(gelu_erf(acc1[mt][4 * q + 0] * WSI + bb.x), ww.x, sc[mt]);
                    sc[mt] = fmaf(gelu_erf(acc1[mt][4 * q + 1] * WSI + bb.y), ww.y, sc[mt]);
                    sc[mt] = fmaf(gelu_erf(acc1[mt][4 * q + 2] * WSI + bb.z), ww.z, sc[mt]);
                    sc[mt] = fmaf(gelu_erf(acc1[mt][4 * q + 3] * WSI + bb.w), ww.w, sc[mt]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float s2 = sc[mt] + __shfl_xor(sc[mt], 32, 64);
                if (lhalf == 0) P[wave * BM32 + mt * 32 + lrow] = s2;
            }
        }
        __syncthreads();
        const int tile = (int)blockIdx.x % m.tiles_x;
        float* pout = m.partial + ((size_t)b * m.tiles_x + tile) * POOL_PSTRIDE;
        if (wave == 0) {                                    // 64 tokens: one per lane; the waves' partials in a fixed order
            float s = (((P[lane] + P[BM32 + lane]) + (P[2 * BM32 + lane] + P[3 * BM32 + lane])) +
                       ((P[4 * BM32 + lane] + P[5 * BM32 + lane]) + (P[6 * BM32 + lane] + P[7 * BM32 + lane]))) + m.att_b2[0];
            if (lane < valid) m.scores[(size_t)b * L + t0 + lane] = s;
            else s = -INFINITY;
            const float mx = wave_max(s);                   // token t0 is always valid: mx is finite
            const float e = expf(s - mx);                   // exp(-inf) = 0 for the rows past L
            E[lane] = e;
            const float ssum = wave_sum(e);
            if (lane == 0) {
                pout[D] = mx;
                pout[D + 1] = ssum;
            }
        }
        __syncthreads();
        {   // vec: thread = (channel pair, 16-token group); the staged ln_f tile is read back (fp32 pairs, or hi + lo halfs of a pair)
            const int c2 = tid & 127, g = tid >> 7;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll 8
            for (int i = 0; i < 16; ++i) {
                const int t = g * 16 + i;
                const float e = E[t];
                float v0, v1;
                if constexpr (AR == AR_X3) {
                    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
                    const char* rowp = reinterpret_cast<const char*>(As + t * RS32) + c2 * 4;
                    const h2_t hi = *reinterpret_cast<const h2_t*>(rowp), lo = *reinterpret_cast<const h2_t*>(rowp + 512);
                    v0 = (float)hi[0] + (float)lo[0], v1 = (float)hi[1] + (float)lo[1];
                } else {
                    const float2 v = *reinterpret_cast<const float2*>(As + t * RS32 + 2 * c2);
                    v0 = v.x, v1 = v.y;
                }
                a0 = fmaf(e, v0, a0);
                a1 = fmaf(e, v1, a1);
            }
            *reinterpret_cast<float2*>(V + g * D + 2 * c2) = make_float2(a0, a1);
        }
        __syncthreads();
        if (tid < D) pout[tid] = (V[tid] + V[D + tid]) + (V[2 * D + tid] + V[3 * D + tid]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// SequenceCNNTransformer, exact fp32: one kernel per encoder layer for everything but the attention itself
//   /root/reference/chimeralm/models/components/transformer.py:64-68 (nn.TransformerEncoderLayer, post-norm, ReLU, no masks)
//       x1  = LN1(h + W_o att + b_o)
//       h'  = LN2(x1 + W_2 relu(W_1 x1 + b_1) + b_2)
//       qkv = W_qkv' h' + b_qkv'                       (the NEXT layer's in_proj; FIRST: only this, on the tile of h as it is)
// Same 64-token tile, weight packing and MFMA loop as tail32_kernel; activations are token-major in HBM ([M, 256] rows).
struct Enc32Args {
    const float* att;         // [M, 256]
    float* h;                 // [M, 256] residual stream (post-norm: normalised), updated in place
    const f32x4 *w_o, *w1, *w2, *w_qkv;
    const float *b_o, *b1, *b2, *b_qkv, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float* qkv;               // [M, 768]
    size_t M;
    float eps;
};

template <int AR = AR_F32>
__device__ __forceinline__ void stage_rows32(const float* __restrict__ src, size_t row0, size_t M, float* T, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = wave + 8 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + r < M) v = *reinterpret_cast<const f32x4*>(src + (row0 + r) * D + lane * 4);
        tile_store4<AR>(T, r, lane * 4, v);
    }
}

template <bool FIRST, int AR = AR_F32>
__global__ __launch_bounds__(512) void enc32_kernel(Enc32Args m) {
    constexpr float WSI = WUNSCALE<AR>;
    extern __shared__ __attribute__((aligned(16))) float smem32[];
    float* As = smem32;
    float* Hs = As + BM32 * RS32;
    float* P1 = smem32 + 2 * BM32 * RS32;
    float* P2 = P1 + 8 * BM32;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * BM32;
    const int valid = m.M - row0 < (size_t)BM32 ? (int)(m.M - row0) : BM32;
    f32x4 ws[2][KS_SET];
    f32x16 acc1[2], acc2[2];
    if constexpr (FIRST) {
        load_wset(wset_ptr(m.w_qkv, 0, D / 8, 0, wave, lane), ws[0]);
        stage_rows32<AR>(m.h, row0, m.M, As, tid);
        __syncthreads();
    } else {
        load_wset(wset_ptr(m.w_o, 0, D / 8, 0, wave, lane), ws[0]);
        stage_rows32<AR>(m.att, row0, m.M, As, tid);
        // Both sublayer sums start from zero and meet their residual once, behind the last MFMA step (as tail32_kernel): summed onto the
        // residual, every step rounds at the residual's magnitude, which a small sublayer (|W_o att| << |h|) pays for in full.
        f32x16 res[2];
        {   // res = h + b_o
            const float* bo = m.b_o + wave * 32 + 4 * lhalf;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const size_t r = row0 + mt * 32 + lrow, rc = r < m.M ? r : m.M - 1;
                const float* row = m.h + rc * D + wave * 32 + 4 * lhalf;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 hv = *reinterpret_cast<const float4*>(row + 8 * q);
                    const float4 bb = *reinterpret_cast<const float4*>(bo + 8 * q);
                    res[mt][4 * q + 0] = hv.x + bb.x;
                    res[mt][4 * q + 1] = hv.y + bb.y;
                    res[mt][4 * q + 2] = hv.z + bb.z;
                    res[mt][4 * q + 3] = hv.w + bb.w;
                    acc2[mt][4 * q + 0] = acc2[mt][4 * q + 1] = acc2[mt][4 * q + 2] = acc2[mt][4 * q + 3] = 0.f;
                }
            }
        }
        __syncthreads();
        product256<false, AR>(As, m.w_o, 0, D / 8, 0, wset_ptr(m.w1, 0, D / 8, 0, wave, lane), wave, lane, ws, acc2);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[mt][r] = acc2[mt][r] * WSI + res[mt][r];
        ln_to_tile<true, AR>(acc2, P1, P2, m.ln1_g, m.ln1_b, m.eps, As, valid, wave, lrow, lhalf);   // As = x1, acc2 = x1
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {                     // x1 waits in `res`; acc2 is fc2's sum
                res[mt][r] = acc2[mt][r];
                acc2[mt][r] = 0.f;
            }
#pragma unroll 1
        for (int j = 0; j < DI / 256; ++j) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[mt][r] = 0.f;
            product256<false, AR>(As, m.w1, j, D / 8, 0, wset_ptr(m.w2, 0, DI / 8, j * 32, wave, lane), wave, lane, ws, acc1);
            {
                const float* b1 = m.b1 + j * 256 + wave * 32 + 4 * lhalf;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 bb = *reinterpret_cast<const float4*>(b1 + 8 * q);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        f32x4 g = {fmaxf(acc1[mt][4 * q + 0] * WSI + bb.x, 0.f), fmaxf(acc1[mt][4 * q + 1] * WSI + bb.y, 0.f),
                                   fmaxf(acc1[mt][4 * q + 2] * WSI + bb.z, 0.f), fmaxf(acc1[mt][4 * q + 3] * WSI + bb.w, 0.f)};
                        tile_store4<AR>(Hs, mt * 32 + lrow, wave * 32 + 8 * q + 4 * lhalf, g);
                    }
                }
            }
            __syncthreads();
            const f32x4* nxt = j + 1 < DI / 256 ? wset_ptr(m.w1, j + 1, D / 8, 0, wave, lane)
                                                : wset_ptr(m.w_qkv ? m.w_qkv : m.w1, 0, D / 8, 0, wave, lane);
            product256<false, AR>(Hs, m.w2, 0, DI / 8, j * 32, nxt, wave, lane, ws, acc2);
            __syncthreads();
        }
        {   // + b_2, LayerNorm-2 -> As and the accumulators; h' leaves as 16 bytes per lane and feature quad
            const float* b2p = m.b2 + wave * 32 + 4 * lhalf;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b2p + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    acc2[mt][4 * q + 0] = (acc2[mt][4 * q + 0] * WSI + bb.x) + res[mt][4 * q + 0];
                    acc2[mt][4 * q + 1] = (acc2[mt][4 * q + 1] * WSI + bb.y) + res[mt][4 * q + 1];
                    acc2[mt][4 * q + 2] = (acc2[mt][4 * q + 2] * WSI + bb.z) + res[mt][4 * q + 2];
                    acc2[mt][4 * q + 3] = (acc2[mt][4 * q + 3] * WSI + bb.w) + res[mt][4 * q + 3];
                }
            }
        }
        ln_to_tile<true, AR>(acc2, P1, P2, m.ln2_g, m.ln2_b, m.eps, As, valid, wave, lrow, lhalf);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                if (mt * 32 + lrow < valid)
                    *reinterpret_cast<float4*>(m.h + (row0 + mt * 32 + lrow) * D + wave * 32 + 4 * lhalf + 8 * q) =
                        make_float4(acc2[mt][4 * q + 0], acc2[mt][4 * q + 1], acc2[mt][4 * q + 2], acc2[mt][4 * q + 3]);
        if (!m.w_qkv) return;                                  // (uniform: after the last layer)
    }
    // qkv = W_qkv As + b_qkv, rows = features: a lane writes 4 consecutive features of its token row
#pragma unroll 1
    for (int nb = 0; nb < D3 / 256; ++nb) {
        zero_acc(acc1);
        product256<false, AR>(As, m.w_qkv, nb, D / 8, 0, wset_ptr(m.w_qkv, nb + 1 < D3 / 256 ? nb + 1 : 0, D / 8, 0, wave, lane), wave, lane,
                              ws, acc1);
        const float* bq = m.b_qkv + nb * 256 + wave * 32 + 4 * lhalf;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bb = *reinterpret_cast<const float4*>(bq + 8 * q);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                if (mt * 32 + lrow < valid)
                    *reinterpret_cast<float4*>(m.qkv + (row0 + mt * 32 + lrow) * D3 + nb * 256 + wave * 32 + 4 * lhalf + 8 * q) =
                        make_float4(acc1[mt][4 * q + 0] * WSI + bb.x, acc1[mt][4 * q + 1] * WSI + bb.y, acc1[mt][4 * q + 2] * WSI + bb.z,
                                    acc1[mt][4 * q + 3] * WSI + bb.w);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// SequenceCNNTransformer, exact fp32: Conv1d(256 -> 256, k = 3, padding = 1) + ReLU + MaxPool1d(2) of the CNN stem
//   /root/reference/chimeralm/models/components/transformer.py:47-58
// as three 256-deep products over ONE staged tile: rows t0 - 1 .. t0 + 64 of the read (zero outside it) lie in LDS once, and tap dk
// reads them shifted by dk rows; weights [3][256][256] (tap-major, each tap in launch_pack_f32t's order).  The pooling pairs are
// adjacent lanes of the accumulator layout (lane = position): one lane exchange, then the even lanes store 16 bytes per feature quad.
struct Conv32Args {
    const float* x;           // [B, Lin, 256]
    const f32x4* w;           // [3] x packed [256, 256]
    const float* bias;
    float* out;               // [B, Lin / 2, 256]
    int B, Lin, tiles_x;
};

template <int AR = AR_F32>
__global__ __launch_bounds__(512) void conv32_kernel(Conv32Args m) {
    constexpr float WSI = WUNSCALE<AR>;
    extern __shared__ __attribute__((aligned(16))) float smem32[];
    float* Xs = smem32;                                     // [66][RS32]: row r = position t0 - 1 + r
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int b = (int)blockIdx.x / m.tiles_x, t0 = ((int)blockIdx.x % m.tiles_x) * BM32, Lin = m.Lin, Lout = Lin / 2;
    f32x4 ws[2][KS_SET];
    f32x16 acc[2];
    load_wset(wset_ptr(m.w, 0, D / 8, 0, wave, lane), ws[0]);
    stage_rows<AR, 1>(Xs, m.x + (size_t)b * Lin * D, t0, Lin, wave, lane);
    zero_acc(acc);
    __syncthreads();
    static_for<0, 3>([&](auto dkc) {
        constexpr int dk = decltype(dkc)::value;
        const f32x4* wdk = m.w + (size_t)dk * (D * D / 4);
        const f32x4* nxt = wset_ptr(dk < 2 ? m.w + (size_t)(dk + 1) * (D * D / 4) : m.w, 0, D / 8, 0, wave, lane);
        product256<false, AR>(Xs + dk * RS32, wdk, 0, D / 8, 0, nxt, wave, lane, ws, acc);
    });
    const float* bp = m.bias + wave * 32 + 4 * lhalf;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 bb = *reinterpret_cast<const float4*>(bp + 8 * q);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float v[4] = {fmaxf(acc[mt][4 * q + 0] * WSI + bb.x, 0.f), fmaxf(acc[mt][4 * q + 1] * WSI + bb.y, 0.f),
                          fmaxf(acc[mt][4 * q + 2] * WSI + bb.z, 0.f), fmaxf(acc[mt][4 * q + 3] * WSI + bb.w, 0.f)};
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], __shfl_xor(v[e], 1, 64));       // positions 2 p, 2 p + 1: adjacent lanes
            const int pos = (t0 + mt * 32 + lrow) >> 1;
            if (!(lrow & 1) && pos < Lout)
                *reinterpret_cast<float4*>(m.out + ((size_t)b * Lout + pos) * D + wave * 32 + 4 * lhalf + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// DNAConvNet, blocks 1 and 2: Conv1d(256 -> 256, k = 7, padding "same") + eval BatchNorm + GELU(erf) + MaxPool1d(4)   (cnn.hip)
// The same implicit GEMM as conv32_kernel with K = 7 x 256: rows t0 - 3 .. t0 + 66 of the block's input (zero outside [0, Lin)) lie
// in LDS once and tap dk reads them shifted by dk rows.  Epilogue per element: bias, then the BatchNorm as a per-channel scale and
// shift (fp32, computed in fp64 at finalize), then GELU -- all on every position, since neither BN nor GELU commutes with the max --
// then the max over the 4 positions of a pooling window, which are 4 adjacent lanes (two lane exchanges).
// POOLSUM (block 2): the pooled rows are not stored; the tile's per-channel sum over its pooled rows < Lout goes to
// partial[b][tile][256] in a fixed order (the head kernel finishes the mean).
struct CnnConvArgs {
    const float* x;           // [B, Lin, 256]
    const f32x4* w;           // [7] x packed [256, 256]
    const float *bias, *bn_scale, *bn_shift;
    float* out;               // [B, Lin / 4, 256]  or  partial [B, tiles_x, 256] (POOLSUM)
    int B, Lin, tiles_x;
};

template <bool POOLSUM, int AR = AR_F32>
__global__ __launch_bounds__(512) void cnn_gemm7_kernel(CnnConvArgs m) {
    constexpr float WSI = WUNSCALE<AR>;
    extern __shared__ __attribute__((aligned(16))) float smem32[];
    float* Xs = smem32;                                     // [70][RS32]: row r = position t0 - 3 + r
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int b = (int)blockIdx.x / m.tiles_x, tile = (int)blockIdx.x % m.tiles_x, t0 = tile * BM32, Lin = m.Lin, Lout = Lin / 4;
    f32x4 ws[2][KS_SET];
    f32x16 acc[2];
    load_wset(wset_ptr(m.w, 0, D / 8, 0, wave, lane), ws[0]);
    stage_rows<AR, cnn::HALO>(Xs, m.x + (size_t)b * Lin * D, t0, Lin, wave, lane);
    zero_acc(acc);
    __syncthreads();
    static_for<0, cnn::K>([&](auto dkc) {
        constexpr int dk = decltype(dkc)::value;
        const f32x4* wdk = m.w + (size_t)dk * (D * D / 4);
        const f32x4* nxt = wset_ptr(dk + 1 < cnn::K ? m.w + (size_t)(dk + 1) * (D * D / 4) : m.w, 0, D / 8, 0, wave, lane);
        product256<false, AR>(Xs + dk * RS32, wdk, 0, D / 8, 0, nxt, wave, lane, ws, acc);
    });
    const int c0 = wave * 32 + 4 * lhalf;
    f32x4 sum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 bb = *reinterpret_cast<const float4*>(m.bias + c0 + 8 * q);
        const float4 sc = *reinterpret_cast<const float4*>(m.bn_scale + c0 + 8 * q);
        const float4 sh = *reinterpret_cast<const float4*>(m.bn_shift + c0 + 8 * q);
        const float bq[4] = {bb.x, bb.y, bb.z, bb.w}, sq[4] = {sc.x, sc.y, sc.z, sc.w}, hq[4] = {sh.x, sh.y, sh.z, sh.w};
        sum[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = gelu_erf((acc[mt][4 * q + e] * WSI + bq[e]) * sq[e] + hq[e]);
                v[e] = fmaxf(v[e], __shfl_xor(v[e], 1, 64));    // positions 4 p .. 4 p + 3: lanes 4 p .. 4 p + 3 of the half-wave
                v[e] = fmaxf(v[e], __shfl_xor(v[e], 2, 64));
            }
            const int pos = (t0 + mt * 32 + lrow) >> 2;
            if constexpr (POOLSUM) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[q][e] += ((lrow & 3) == 0 && pos < Lout) ? v[e] : 0.f;
            } else {
                if ((lrow & 3) == 0 && pos < Lout)
                    *reinterpret_cast<float4*>(m.out + ((size_t)b * Lout + pos) * D + c0 + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    if constexpr (POOLSUM) {
        // the 8 window leaders of each half-wave (lanes 0, 4, .., 28; the others hold 0) in a fixed tree, then lane 0 / 32 writes
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = sum[q][e];
                s += __shfl_xor(s, 4, 64);
                s += __shfl_xor(s, 8, 64);
                s += __shfl_xor(s, 16, 64);
                sum[q][e] = s;
            }
        if (lrow == 0) {
            float* po = m.out + ((size_t)b * m.tiles_x + tile) * D + c0;
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(po + 8 * q) = make_float4(sum[q][0], sum[q][1], sum[q][2], sum[q][3]);
        }
    }
}

// W [N][K] row-major fp32 -> [N / 256][8 waves][K / 8 k-steps][64 lanes] float4: lane (lrow, lhalf) of wave w holds
// W[nb * 256 + w * 32 + lrow][8 s + 4 lhalf + 0..3]
__global__ __launch_bounds__(256) void pack_f32t_kernel(const float* __restrict__ w, f32x4* __restrict__ out, int N, int K) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)N * K / 4;
    if (i >= total) return;
    const int lane = (int)(i & 63), lrow = lane & 31, lhalf = lane >> 5;
    const size_t rest = i >> 6;
    const int ksteps = K / 8, s = (int)(rest % ksteps), nw = (int)(rest / ksteps);       // nw = nb * 8 + wave
    const float* src = w + (size_t)(nw * 32 + lrow) * K + 8 * s + 4 * lhalf;
    out[i] = f32x4{src[0], src[1], src[2], src[3]};
}

// AR_X3: W [N][K] -> [N / 256][8 waves][K / 16 k-steps][hi | lo][64 lanes] x 8 halfs: lane (lrow, lhalf) of wave w holds
// fp16(1024 W[nb * 256 + w * 32 + lrow][16 s + 8 lhalf + 0..7]) and, in the next fragment, the fp16 of what that rounding left
__global__ __launch_bounds__(256) void pack_x3_kernel(const float* __restrict__ w, f32x4* __restrict__ out, int N, int K) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)N * K / 4;     // fragments: N K / 8 hi + N K / 8 lo
    if (i >= total) return;
    const int lane = (int)(i & 63), lrow = lane & 31, lhalf = lane >> 5;
    const size_t rest = i >> 6;
    const int frags = K / 8, f = (int)(rest % frags), nw = (int)(rest / frags), s = f >> 1, plane = f & 1;
    const float* src = w + (size_t)(nw * 32 + lrow) * K + 16 * s + 8 * lhalf;
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = src[j] * X3_WS;
        const _Float16 hi = (_Float16)__builtin_amdgcn_fmed3f(x, -65504.f, 65504.f);       // (|w| > 64: saturating, like split4)
        o[j] = plane ? (_Float16)__builtin_amdgcn_fmed3f(x - (float)hi, -65504.f, 65504.f) : hi;
    }
    out[i] = __builtin_bit_cast(f32x4, o);
}

void launch_pack_x3(const float* w, void* out, int n, int k, hipStream_t st) {
    const size_t total = (size_t)n * k / 4;
    hipLaunchKernelGGL(pack_x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, reinterpret_cast<f32x4*>(out), n, k);
}

void launch_pack_f32t(const float* w, void* out, int n, int k, hipStream_t st) {
    const size_t total = (size_t)n * k / 4;
    hipLaunchKernelGGL(pack_f32t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, reinterpret_cast<f32x4*>(out), n, k);
}

// f(the arithmetic as a compile-time constant): x3 = the products as three fp16 MFMAs on hi + lo halfs (weights from launch_pack_x3)
// instead of the fp32 MFMA
template <class F>
void with_arith(bool x3, F f) {
    if (x3) f(std::integral_constant<int, AR_X3>{});
    else f(std::integral_constant<int, AR_F32>{});
}

// Exactly one of `score` / `w_in_next` is given: score (the last block) -- ln_f + pooling scores + per-64-token-tile pooling partials
// follow on the tile; w_in_next (every other block) -- the next block's LayerNorm-1 + in_proj.  There is no tail without either.
void launch_tail32(const float* y, float* h, const void* w_out, const void* w_fc1, const void* w_fc2, const void* w_in_next,
                   const float* b_out, const float* b_fc1, const float* b_fc2, const float* b_in_next, const float* ln2_g,
                   const float* ln2_b, const float* n_g, const float* n_b, float* z, int B, int L, int Lp, float eps, hipStream_t st,
                   bool x3, const int* p0, const Tail32Score* score, const unsigned char* ids8, const float* emb) {
    Tail32Args m{y, h, reinterpret_cast<const f32x4*>(w_out), reinterpret_cast<const f32x4*>(w_fc1), reinterpret_cast<const f32x4*>(w_fc2),
                 reinterpret_cast<const f32x4*>(score ? score->w1 : w_in_next), b_out, b_fc1, b_fc2, score ? score->b1 : b_in_next, ln2_g, ln2_b,
                 score ? score->lnf_g : n_g, score ? score->lnf_b : n_b, z, B, L, Lp,
                 (L + BM32 - 1) / BM32, eps, p0, score ? score->w2 : nullptr, score ? score->b2 : nullptr, score ? score->scores : nullptr,
                 score ? score->partial : nullptr, ids8, emb};
    const size_t lds = (size_t)(2 * BM32 * RS32 + 2 * 8 * BM32) * sizeof(float);
    static_assert(8 * BM32 + BM32 + 4 * D <= BM32 * RS32, "score stage: P / E / V fit the Hs region");
    const dim3 grid((unsigned)(m.tiles_x * B));
    const dim3 block(512);
    with_arith(x3, [&](auto ar) {
        if (score) launch_lds<tail32_kernel<T32_SCORE, ar()>>(grid, block, lds, st, m);
        else launch_lds<tail32_kernel<T32_INPROJ, ar()>>(grid, block, lds, st, m);
    });
}

// FIRST (att == null): qkv of the tile of h as it is (the first layer's in_proj); otherwise the whole layer after its attention,
// and -- w_qkv != null -- the next layer's in_proj.  Weights in launch_pack_f32t's order.
void launch_enc32(const float* att, float* h, const void* w_o, const void* w1, const void* w2, const void* w_qkv, const float* b_o,
                  const float* b1, const float* b2, const float* b_qkv, const float* ln1_g, const float* ln1_b, const float* ln2_g,
                  const float* ln2_b, float* qkv, size_t M, float eps, hipStream_t st, bool x3) {
    Enc32Args m{att, h, reinterpret_cast<const f32x4*>(w_o), reinterpret_cast<const f32x4*>(w1), reinterpret_cast<const f32x4*>(w2),
                reinterpret_cast<const f32x4*>(w_qkv), b_o, b1, b2, b_qkv, ln1_g, ln1_b, ln2_g, ln2_b, qkv, M, eps};
    const size_t lds = (size_t)(2 * BM32 * RS32 + 2 * 8 * BM32) * sizeof(float);
    const dim3 grid((unsigned)((M + BM32 - 1) / BM32)), block(512);
    with_arith(x3, [&](auto ar) {
        if (!att) launch_lds<enc32_kernel<true, ar()>>(grid, block, lds, st, m);
        else launch_lds<enc32_kernel<false, ar()>>(grid, block, lds, st, m);
    });
}

// x [B, Lin, 256] -> relu(conv1d_k3(x) + bias) pooled by 2 -> out [B, Lin / 2, 256]; w: three taps, each packed by launch_pack_f32t
void launch_conv32(const float* x, const void* w, const float* bias, float* out, int B, int Lin, hipStream_t st, bool x3) {
    Conv32Args m{x, reinterpret_cast<const f32x4*>(w), bias, out, B, Lin, (Lin + BM32 - 1) / BM32};
    const size_t lds = (size_t)(BM32 + 2) * RS32 * sizeof(float);
    const dim3 grid((unsigned)(m.tiles_x * B)), block(512);
    with_arith(x3, [&](auto ar) { launch_lds<conv32_kernel<ar()>>(grid, block, lds, st, m); });
}

// DNAConvNet block 1 / 2 (cnn.hip): x [B, Lin, 256] -> maxpool4(gelu(bn(conv1d_k7(x) + bias))) -> out [B, Lin / 4, 256], or with
// `partial` the per-64-row-tile channel sums of those pooled rows -> partial [B, ceil(Lin / 4 / 16), 256]; w: seven taps, each
// packed by launch_pack_f32t (x3: launch_pack_x3)
void launch_cnn_gemm7(const float* x, const void* w, const float* bias, const float* bn_scale, const float* bn_shift, float* out,
                      bool partial, int B, int Lin, hipStream_t st, bool x3) {
    const int Lout = Lin / 4;
    CnnConvArgs m{x, reinterpret_cast<const f32x4*>(w), bias, bn_scale, bn_shift, out, B, Lin, (4 * Lout + BM32 - 1) / BM32};
    const size_t lds = (size_t)(BM32 + 2 * cnn::HALO) * RS32 * sizeof(float);
    const dim3 grid((unsigned)(m.tiles_x * B)), block(512);
    with_arith(x3, [&](auto ar) {
        if (partial) launch_lds<cnn_gemm7_kernel<true, ar()>>(grid, block, lds, st, m);
        else launch_lds<cnn_gemm7_kernel<false, ar()>>(grid, block, lds, st, m);
    });
}

}  // namespace clm
