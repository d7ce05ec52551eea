// pool_train.hip -- the attention pooling of the Hyena head as a trainable layer: forward and backward on caller-supplied weights
// (the frozen-backbone fine-tune, chimeralm_amd/headtrain.py).  Reference arithmetic:
//   /root/reference/chimeralm/models/components/hyena.py:117-132, per read, with x_t = ln_f(h_t) (ln_f is backbone: frozen)
//     u_t = W1 x_t + b1,  g_t = gelu_erf(u_t) (the backward: u_t normal_cdf(u_t)),  s_t = w2 . g_t + b2,  a = softmax_t(s) over ALL L,  p = sum_t a_t x_t
//   backward, given dp = dloss/dp:
//     ds_t = a_t ((x_t - p) . dp)          (sum_t a_t (x_t . dp) = p . dp: no reduction pass of its own)
//     dw2 = sum ds_t g_t,  db2 = sum ds_t,  du_t = ds_t w2 * gelu'(u_t),  gelu'(u) = Phi(u) + u phi(u)
//     db1 = sum du_t,  dW1 = sum_t du_t x_t^T      (256 x 256, reduced over all B L tokens)
//
// Forward: the engine's own separate kernels (score GEMM, softmax statistics, pooling partials) on a per-call packing of W1 -- the
// weights change every step -- plus pool_combine_kernel, which adds the partials in head_mlp_kernel's fixed order.
//
// Backward (pool_bwd_kernel), exact fp32 on v_mfma_f32_32x32x2_f32, the 64-token tile of mfma32_common.h, 8 waves:
//   rows -> ln_to_tile -> x tile (LDS, token-major);  u = W1 x on the same packed fragments as product256 (wave w: features 32 w .. 32 w + 31, lane = token);
//   (x_t - p) . dp as a 256-wide row dot across the eight waves -> ds_t;  ds_t g and du staged feature-major in LDS ([256][RSD]):
//   their row sums are dw2 / db1 of the tile, and du is the A operand of dW1 += du . x (K = the tile's 64 tokens; the x tile is B).
//   A workgroup keeps its 256 x 256 share of dW1 in accumulators (wave w: rows 32 w .. 32 w + 31 x 8 column tiles = 128 registers
//   per lane) across ALL the tiles it owns -- tile i goes to workgroup i mod grid, grid <= POOL_BWD_GRID -- and writes ONE partial
//   [dW1 | db1 | dw2 | db2]; pool_bwd_reduce_kernel adds the partials in workgroup order: out = beta out + sum.  No floating-point
//   atomics: the same inputs give the same bits.  Rows past L are zero in the x tile and have ds = 0: they contribute nothing.
#include "chimeralm_hip.h"
#include "clm_common.h"

#include "mfma32_common.h"

namespace clm {

namespace {

constexpr int RSD = 68;           // row stride (floats) of the feature-major du tile [256][64 tokens]: 16 rows of a ds_read_b128 lane
                                  // group fall on 16 different 16-byte bank groups (68 = 4 mod 64)
constexpr float INV_SQRT_2PI = 0.3989422804014327f;

struct PoolBwdArgs {
    const float* rows;            // [B, L, 256] final residual rows (before ln_f)
    const float *lnf_g, *lnf_b;
    const f32x4* w1;              // attention.0.weight packed by launch_pack_f32t
    const float *b1, *w2;
    const float *scores, *stats;  // [B, L], [B, 2] = (max, sum) of the forward
    const float *pooled, *dpooled;   // [B, 256]
    float* partial;               // [grid][POOL_BWD_PSTRIDE]
    int B, L, tiles_x, tiles;
    float eps;
};

// sum of the 64 tokens of feature row (tid >> 1) of the staged tile: two threads per row, 32 tokens each, fixed order
__device__ __forceinline__ float row_sum64(const float* Du, int tid) {
    const float* p = Du + (tid >> 1) * RSD + (tid & 1) * 32;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * i);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    return s + __shfl_xor(s, 1, 64);
}

}  // namespace

__global__ __launch_bounds__(512) void pool_bwd_kernel(PoolBwdArgs m) {
    extern __shared__ __attribute__((aligned(16))) float smem_pb[];
    float* As = smem_pb;                                    // x = ln_f(rows) tile [64][RS32], token-major
    float* Du = As + BM32 * RS32;                           // ds g, then du: [256 features][RSD], feature-major
    float* P1 = Du + D * RSD;                               // LayerNorm partials, then the row-dot partials [8][64]
    float* P2 = P1 + 8 * BM32;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int L = m.L;
    f32x16 dacc[8];                                         // dW1 rows 32 wave .. + 31 (accumulator rows), columns 32 ct + lrow
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[ct][r] = 0.f;
    float dw2_acc = 0.f, db1_acc = 0.f, db2_acc = 0.f;      // feature tid >> 1 (both threads of the pair hold the same sums)
    const f32x4* const w1frag = wset_ptr(m.w1, 0, D / 8, 0, wave, lane);
    const int c0 = wave * 32 + 4 * lhalf;                   // this lane's features: c0 + 8 q + e  <->  accumulator row r = 4 q + e

#pragma unroll 1
    for (int tile = blockIdx.x; tile < m.tiles; tile += gridDim.x) {
        const int b = tile / m.tiles_x, t0 = (tile % m.tiles_x) * BM32;
        const int valid = L - t0 < BM32 ? L - t0 : BM32;
        f32x16 acc[2];
        // ---- 1. rows -> accumulator layout (lane = token, 16 features), ln_f -> As (and acc: KEEP)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int t = t0 + mt * 32 + lrow, tc = t < L ? t : L - 1;
            const float* row = m.rows + ((size_t)b * L + tc) * D + c0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 hv = *reinterpret_cast<const float4*>(row + 8 * q);
                acc[mt][4 * q + 0] = hv.x, acc[mt][4 * q + 1] = hv.y, acc[mt][4 * q + 2] = hv.z, acc[mt][4 * q + 3] = hv.w;
            }
        }
        ln_to_tile<true>(acc, P1, P2, m.lnf_g, m.lnf_b, m.eps, As, valid, wave, lrow, lhalf);
        // ---- 2. (x_t - p) . dp: this wave's 32 features of both tokens of the lane -> P1[wave][token]  (P1's LayerNorm sums were
        //         read before ln_to_tile's last barrier)
        {
            const float* pp = m.pooled + (size_t)b * D + c0;
            const float* dp = m.dpooled + (size_t)b * D + c0;
            float dot[2] = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 p4 = *reinterpret_cast<const float4*>(pp + 8 * q), d4 = *reinterpret_cast<const float4*>(dp + 8 * q);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    dot[mt] = fmaf(acc[mt][4 * q + 0] - p4.x, d4.x, dot[mt]);
                    dot[mt] = fmaf(acc[mt][4 * q + 1] - p4.y, d4.y, dot[mt]);
                    dot[mt] = fmaf(acc[mt][4 * q + 2] - p4.z, d4.z, dot[mt]);
                    dot[mt] = fmaf(acc[mt][4 * q + 3] - p4.w, d4.w, dot[mt]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float d2 = dot[mt] + __shfl_xor(dot[mt], 32, 64);
                if (lhalf == 0) P1[wave * BM32 + mt * 32 + lrow] = d2;
            }
        }
        // ---- 3. u - b1 = W1 x
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        product256_ring(As, w1frag, lrow, lhalf, acc);
        __syncthreads();                                    // the row-dot partials of all waves
        // ---- 4. ds_t of the lane's two tokens (every wave computes all 64: no second hand-over)
        float ds[2];
        {
            const float mx = m.stats[2 * b], inv = 1.0f / m.stats[2 * b + 1];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int tl = mt * 32 + lrow;
                const float dot = ((P1[tl] + P1[BM32 + tl]) + (P1[2 * BM32 + tl] + P1[3 * BM32 + tl])) +
                                  ((P1[4 * BM32 + tl] + P1[5 * BM32 + tl]) + (P1[6 * BM32 + tl] + P1[7 * BM32 + tl]));
                const bool ok = tl < valid;
                const float s = ok ? m.scores[(size_t)b * L + t0 + tl] : 0.f;
                ds[mt] = ok ? expf(s - mx) * inv * dot : 0.f;
            }
            if (wave == 0 && lhalf == 0) db2_acc += ds[0] + ds[1];
        }
        // ---- 5. g and gelu'(u); ds g -> Du (row sums: dw2), acc <- du = ds w2 gelu'(u)
        {
            const float* b1p = m.b1 + c0;
            const float* w2p = m.w2 + c0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = *reinterpret_cast<const float4*>(b1p + 8 * q), ww = *reinterpret_cast<const float4*>(w2p + 8 * q);
                const float bq[4] = {bb.x, bb.y, bb.z, bb.w}, wq[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const float u = acc[mt][4 * q + e] + bq[e];
                        const float cdf = normal_cdf(u);           // 0.5 erfc(-u / sqrt 2): exact in the far tail (clm_common.h)
                        const float pdf = INV_SQRT_2PI * expf(-0.5f * u * u);
                        Du[(c0 + 8 * q + e) * RSD + mt * 32 + lrow] = ds[mt] * (u * cdf);
                        acc[mt][4 * q + e] = ds[mt] * wq[e] * fmaf(u, pdf, cdf);
                    }
                __builtin_amdgcn_sched_barrier(0);          // (one feature quad at a time: erfcf's temporaries of all 32 elements do not fit)
            }
        }
        __syncthreads();
        dw2_acc += row_sum64(Du, tid);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) Du[(c0 + 8 * q + e) * RSD + mt * 32 + lrow] = acc[mt][4 * q + e];
        __syncthreads();
        db1_acc += row_sum64(Du, tid);
        // ---- 6. dW1 += du . x over the tile's 64 tokens.  The reduction index may be permuted freely: k-step i of 16-token group j
        //         pairs token 16 j + i (lanes 0-31) with token 16 j + 8 + i (lanes 32-63) -- A is two 16-byte loads per group, and
        //         the two half-waves read x rows 8 apart (8 RS32 = 32 mod 64 banks)
        {
            const float* ap = Du + (wave * 32 + lrow) * RSD + 8 * lhalf;
            const float* bp = As + (8 * lhalf) * RS32 + lrow;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + 16 * j), a1 = *reinterpret_cast<const f32x4*>(ap + 16 * j + 4);
                const float a[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float* brow = bp + (16 * j + i) * RS32;
#pragma unroll
                    for (int ct = 0; ct < 8; ++ct) dacc[ct] = mfma32(a[i], brow[ct * 32], dacc[ct]);
                }
            }
        }
        // (the next tile's first LDS writes are ln_to_tile's P1 sums, which nothing above still reads -- every wave passed the du
        //  barrier after its row dots -- and As / Du are written only behind ln_to_tile's barriers)
    }

    // ---- the workgroup's partial: dW1 [256][256] | db1 [256] | dw2 [256] | db2.  (The lane's indices are taken afresh from mbcnt: derived
    //      from the ones above they would be held in registers across the whole tile loop, which has none to spare.)
    {
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), lr = ln & 31, lh = ln >> 5;
        float* out = m.partial + (size_t)blockIdx.x * POOL_BWD_PSTRIDE;
        float* orow = out + (size_t)(wave * 32 + 4 * lh) * D + lr;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) orow[acc_row(r, 0) * D + ct * 32] = dacc[ct][r];
        const int f = wave * 32 + (ln >> 1);                // = tid >> 1
        if (!(ln & 1)) {
            out[D * D + f] = db1_acc;
            out[D * D + D + f] = dw2_acc;
        }
        if (wave == 0) {
            const float s = wave_sum(lh == 0 ? db2_acc : 0.f);
            if (ln == 0) out[D * D + 2 * D] = s;
        }
    }
}

// out = beta out + sum over the workgroups' partials, in workgroup order (beta = 0: out is not read)
__global__ __launch_bounds__(256) void pool_bwd_reduce_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ d_w1,
                                                              float* __restrict__ d_b1, float* __restrict__ d_w2,
                                                              float* __restrict__ d_b2, float beta) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= POOL_BWD_PSTRIDE) return;
    float s = 0.f;
    for (int w = 0; w < nparts; ++w) s += partial[(size_t)w * POOL_BWD_PSTRIDE + i];
    float* dst = i < D * D ? d_w1 + i : (i < D * D + D ? d_b1 + (i - D * D) : (i < D * D + 2 * D ? d_w2 + (i - D * D - D) : d_b2));
    *dst = beta != 0.f ? fmaf(beta, *dst, s) : s;
}

// pooled[b][c] = the POOL_SPLIT * 4 partials of pool_kernel in head_mlp_kernel's order: splits outer, waves inner
__global__ __launch_bounds__(256) void pool_combine_kernel(const float* __restrict__ partial, float* __restrict__ pooled) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = partial + (size_t)b * POOL_SPLIT * 4 * D + tid;
    float acc = 0.f;
    for (int s = 0; s < POOL_SPLIT * 4; ++s) acc += p[(size_t)s * D];
    pooled[(size_t)b * D + tid] = acc;
}

void launch_pool_combine(const float* partial, float* pooled, int B, hipStream_t st) {
    hipLaunchKernelGGL(pool_combine_kernel, dim3(B), dim3(256), 0, st, partial, pooled);
}

int pool_bwd_grid(int B, int L) {
    const long long tiles = (long long)B * ((L + BM32 - 1) / BM32);
    return tiles < POOL_BWD_GRID ? (int)tiles : POOL_BWD_GRID;
}

void launch_pool_bwd(const float* rows, const float* lnf_g, const float* lnf_b, const void* w1_packed, const float* b1, const float* w2,
                     const float* scores, const float* stats, const float* pooled, const float* dpooled, float* partial, float* d_w1,
                     float* d_b1, float* d_w2, float* d_b2, float beta, int B, int L, float eps, hipStream_t st) {
    const int tiles_x = (L + BM32 - 1) / BM32, grid = pool_bwd_grid(B, L);
    PoolBwdArgs m{rows, lnf_g, lnf_b, reinterpret_cast<const f32x4*>(w1_packed), b1, w2, scores, stats, pooled, dpooled, partial,
                  B, L, tiles_x, tiles_x * B, eps};
    const size_t lds = (size_t)(BM32 * RS32 + D * RSD + 2 * 8 * BM32) * sizeof(float);
    launch_lds<pool_bwd_kernel>(dim3((unsigned)grid), dim3(512), lds, st, m);
    hipLaunchKernelGGL(pool_bwd_reduce_kernel, dim3((POOL_BWD_PSTRIDE + 255) / 256), dim3(256), 0, st, partial, grid, d_w1, d_b1, d_w2,
                       d_b2, beta);
}

}  // namespace clm
