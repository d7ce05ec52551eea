// cnn_train.hip -- DNAConvNet in training mode on MI355X: forward on batch statistics and the full backward, on the CALLER's current
// parameters (chimeralm_amd/cnntrain.py), behind the clm_cnn_train_* C ABI.  Exact fp32 throughout (v_mfma_f32_32x32x2_f32).
//
// Reference: chimeralm/models/components/cnn.py in train(), production shape (configs/model/cnn.yaml).  Rows are token-major
// [B, L_i, 256], L_0 = L, L_{i+1} = floor(L_i / 4); pads are ordinary tokens.  Block i = 0, 1, 2:
//   z  = conv1d_same(x_i; W_i, b_i) on ALL L_i positions      (x_0 = embedding rows)
//   mu, v = mean and biased variance of z[:, :, c] over all B L_i positions (those no pooling window covers included)
//   xh = (z - mu) rstd, rstd = 1 / sqrt(v + 1e-5);   y = gelu_erf(g xh + beta)
//   p[b, j, c] = max_{r < 4} y[b, 4 j + r, c], choice = the LOWEST r that attains it;   x_{i+1} = p keep scale
// pooled[b] = mean_j x_3[b, j, :].  Backward from dpooled: mean, mask, max-pool (to `choice` only), gelu', then
//   dz = g rstd (dy - mean(dy) - xh mean(dy xh)),  dg = sum dy xh,  dbeta = sum dy,  db = sum dz,
//   dW[co, ci, k] = sum_{b, t} dz[b, t, co] x[b, t + k - 3, ci],  dx = conv1d_same(dz; W flipped in k, ci / co exchanged),
//   d embedding[tok] = sum of dx_0 over the positions holding tok (row 4 zero).
//
// Kernels (all cnn_train_*).  No floating-point atomics, every reduction in a fixed order: the same inputs give the same bits.
//   table, conv0      block 0 needs no GEMM: T[dk][tok][co] = W_0[:, :, dk] . E[tok] (fp64 sums, rebuilt per step), z_0 by lookup.
//   gemm7             blocks 1, 2 and every dx: cnn_gemm7_kernel's implicit GEMM (K = 7 x 256, halo rows in LDS once) with a raw
//                     epilogue (+ bias) over all L_i positions and one accumulator per tap; weights packed per step (pack: forward,
//                     and flipped / transposed).
//   stats, stats_final  per-channel sums of z and z^2 in fp64 per workgroup, combined in workgroup order (as four slices of the
//                     workgroups, each in order, added in slice order: every small reduction here runs so) -> mu, v, rstd.
//   bnpool, mean      BN, GELU, pool, choice (one byte per pooled element), mask; block 2's mean over positions in order.
//   dy                dy at the chosen positions (one value per pooled element) and the fp64 partials of sum dy, sum dy xh.
//   dz                dz on all positions;  db = its column sums (stats again).
//   dw, dw_reduce     split-K MFMA: workgroup (g, tap) keeps its 256 x 256 share of dW[:, :, tap] in accumulators across the tiles
//                     it owns (tile i -> workgroup i mod G), A = the dz tile feature-major, B = the x tile shifted by the tap;
//                     one partial per workgroup, added in workgroup order in fp64.
//   dt, dt_reduce     block 0: dT[dk][tok][co] = sum of dz_0[b, t, co] over ids[b, t + dk - 3] = tok; one thread per channel walks
//                     the workgroup's positions into a 7 x 13 x 256 LDS table (row 12: outside the read); partials in order.
//   dw0, de           dW_0 and d embedding from dT: two tiny products in fp64.
// Shared with inference: the net's constants and conv0's two staging steps (cnn_common.h), gemm7's input tile (mfma32_common.h stage_rows).
#include <string>

#include "chimeralm_hip.h"
#include "handle_host.h"
#include "cnn_common.h"
#include "mfma32_common.h"

namespace clm {
namespace {

constexpr int CT_PT0 = 256;                        // conv0: positions per workgroup
constexpr int CT_RSD = 68;                         // row stride (floats) of the feature-major dz tile [256][64] (pool_train.hip RSD)
constexpr int CT_DW_GRID = 36;                     // dw: workgroups per tap at most (x 7 taps = 252 of the 256 CUs)
constexpr int CT_STAT_GRID = 512;                  // stats / dy: workgroups at most
constexpr int CT_DT_GRID = 256;                    // dt: workgroups at most
constexpr int CT_DT_SUB = 512;                     // dt: positions whose table rows are staged in LDS at a time
constexpr int CT_SLICES = 4;                       // the small reductions: 1,024 threads = 256 columns x 4 slices of the summed index
constexpr int CT_TSIZE = cnn::K * cnn::VOC * D;        // floats of T / dT
constexpr float CT_INV_SQRT_2PI = 0.3989422804014327f;

// (the cdf is clm_common.h normal_cdf, 0.5 erfc(-u / sqrt 2), shared with pool_train.hip; the comment there says why)
__device__ __forceinline__ float ct_gelu_grad(float u) {
    const float cdf = normal_cdf(u);
    const float pdf = CT_INV_SQRT_2PI * expf(-0.5f * u * u);
    return fmaf(u, pdf, cdf);
}
// the small reductions run as CT_SLICES partial sums per column, each in index order, added in slice order: red [CT_SLICES][256]
__device__ __forceinline__ double ct_combine(double v, double* red, int slice, int c) {
    red[slice * D + c] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < CT_SLICES; ++i) t += red[i * D + c];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float ct_y(float z, float mu, float rstd, float g, float beta) {
    const float u = g * ((z - mu) * rstd) + beta;
    return u * normal_cdf(u);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ block 0: table and lookup
// grid 7 x 12 (dk, tok), 1,024 threads (co, slice of ci): T[dk][tok][co] = sum_ci W[co][ci][dk] E[tok][ci] in fp64
__global__ __launch_bounds__(1024) void cnn_train_table_kernel(const float* __restrict__ E, const float* __restrict__ W, float* __restrict__ T) {
    __shared__ float Es[D];
    __shared__ double red[CT_SLICES * D];
    const int dk = blockIdx.x / cnn::VOC, tok = blockIdx.x % cnn::VOC, co = threadIdx.x & (D - 1), slice = threadIdx.x >> 8;
    if (slice == 0) Es[co] = E[(size_t)tok * D + co];
    __syncthreads();
    const float* w = W + (size_t)co * D * cnn::K + dk;
    double s = 0.0;
    for (int ci = slice * (D / CT_SLICES); ci < (slice + 1) * (D / CT_SLICES); ++ci) s += (double)w[(size_t)ci * cnn::K] * (double)Es[ci];
    s = ct_combine(s, red, slice, co);
    if (slice == 0) T[((size_t)dk * cnn::VOC + tok) * D + co] = (float)s;
}

// grid (ceil(L / CT_PT0), B), 512 threads: thread = (channel, half of the workgroup's positions); z_0 on every position < L
__global__ __launch_bounds__(512) void cnn_train_conv0_kernel(const unsigned char* __restrict__ ids8, int Lp, const float* __restrict__ table,
                                                              const float* __restrict__ bias, float* __restrict__ z, int L) {
    extern __shared__ __attribute__((aligned(16))) float smem_ct0[];
    float* Ts = smem_ct0;                                      // [K][TROWS][256]
    int* idl = reinterpret_cast<int*>(Ts + cnn::K * cnn::TROWS * D);   // [PT0 + 2 HALO]: LDS row offset of token t0 - 3 + i
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * CT_PT0;
    cnn::stage_table(Ts, table, tid);
    cnn::stage_token_rows(idl, ids8 + (size_t)b * Lp, t0 - cnn::HALO, CT_PT0 + 2 * cnn::HALO, L, tid, D);
    __syncthreads();
    const int c = tid & (D - 1), half = tid >> 8;
    const float bc = bias[c];
    const float* Tc = Ts + c;
    const int tbeg = t0 + half * (CT_PT0 / 2), tend = tbeg + CT_PT0 / 2 < L ? tbeg + CT_PT0 / 2 : L;
    for (int t = tbeg; t < tend; ++t) {
        const int* id = idl + (t - t0);                        // token t + dk - 3 -> id[dk]
        float v = bc;
#pragma unroll
        for (int dk = 0; dk < cnn::K; ++dk) v += Tc[dk * cnn::TROWS * D + id[dk]];
        z[((size_t)b * L + t) * D + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ weights per step
// W [co][ci][7] -> seven taps in launch_pack_f32t's order.  flip = 0: tap dk = W[:, :, dk] as [n = co][k = ci] (the forward);
// flip = 1: tap dk = W[:, :, 6 - dk] as [n = ci][k = co] (dx)
__global__ __launch_bounds__(256) void cnn_train_pack_kernel(const float* __restrict__ W, f32x4* __restrict__ out, int flip) {
    const int i = blockIdx.x * 256 + threadIdx.x;              // < 7 * 256 * 256 / 4
    const int tap = i / (D * D / 4), j = i % (D * D / 4), lane = j & 63, lrow = lane & 31, lhalf = lane >> 5, rest = j >> 6;
    const int s = rest % (D / 8), nw = rest / (D / 8), n = nw * 32 + lrow, k0 = 8 * s + 4 * lhalf;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        v[e] = flip ? W[((size_t)(k0 + e) * D + n) * cnn::K + (cnn::K - 1 - tap)] : W[((size_t)n * D + k0 + e) * cnn::K + tap];
    out[i] = v;
}

// ------------------------------------------------------------------------------------------------ implicit GEMM, raw epilogue
struct CnnTrainGemmArgs {
    const float* x;           // [B, Lin, 256]
    const f32x4* w;           // [7] x packed [256, 256]
    const float* bias;        // [256] or null
    float* out;               // [B, Lin, 256]
    int Lin, tiles_x;
};

__global__ __launch_bounds__(512) void cnn_train_gemm7_kernel(CnnTrainGemmArgs m) {
    extern __shared__ __attribute__((aligned(16))) float smem_ctg[];
    float* Xs = smem_ctg;                                   // [70][RS32]: row r = position t0 - 3 + r
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int b = (int)blockIdx.x / m.tiles_x, t0 = ((int)blockIdx.x % m.tiles_x) * BM32, Lin = m.Lin;
    f32x16 tot[2];
    stage_rows<AR_F32, cnn::HALO>(Xs, m.x + (size_t)b * Lin * D, t0, Lin, wave, lane);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[mt][r] = 0.f;
    __syncthreads();
    // one accumulator per tap, the seven added at the end of each: a chain of 128 MFMAs where one accumulator for all K = 1,792
    // would be a chain of 896 -- the rounding of a running fp32 sum grows with its length, and training reads z closer than
    // inference does
#pragma unroll 1
    for (int dk = 0; dk < cnn::K; ++dk) {
        f32x16 acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        product256_ring(Xs + dk * RS32, wset_ptr(m.w + (size_t)dk * (D * D / 4), 0, D / 8, 0, wave, lane), lrow, lhalf, acc);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) tot[mt] += acc[mt];
    }
    const int c0 = wave * 32 + 4 * lhalf;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m.bias) bb = *reinterpret_cast<const float4*>(m.bias + c0 + 8 * q);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int t = t0 + mt * 32 + lrow;
            if (t < Lin)
                *reinterpret_cast<float4*>(m.out + ((size_t)b * Lin + t) * D + c0 + 8 * q) =
                    make_float4(tot[mt][4 * q + 0] + bb.x, tot[mt][4 * q + 1] + bb.y, tot[mt][4 * q + 2] + bb.z, tot[mt][4 * q + 3] + bb.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------ column sums in fp64
// 256 threads (channel); workgroup w sums rows [w chunk, (w + 1) chunk) of v [n][256]: partial[w][0][c] = sum v, [w][1][c] = sum v^2
__global__ __launch_bounds__(256) void cnn_train_stats_kernel(const float* __restrict__ v, size_t n, size_t chunk, double* __restrict__ partial) {
    const int c = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    double s = 0.0, q = 0.0;
    for (size_t r = r0; r < r1; ++r) {
        const double x = (double)v[r * D + c];
        s += x;
        q += x * x;
    }
    partial[((size_t)blockIdx.x * 2 + 0) * D + c] = s;
    partial[((size_t)blockIdx.x * 2 + 1) * D + c] = q;
}

// the partials in workgroup order.  mode 0 (forward): mean, biased variance and rstd of n values per channel, also to the caller's
// mean_out / var_out;  mode 1 (dy): o0 = m1 = S0 / n, o1 = m2 = S1 / n, and dbeta = beta_acc dbeta + S0, dg = beta_acc dg + S1;
// mode 2 (db): db = beta_acc db + S0
__global__ __launch_bounds__(1024) void cnn_train_stats_final_kernel(const double* __restrict__ partial, int parts, double n, int mode,
                                                                    float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
                                                                    float* __restrict__ g0, float* __restrict__ g1, float beta_acc) {
    __shared__ double red[CT_SLICES * D];
    const int c = threadIdx.x & (D - 1), slice = threadIdx.x >> 8, per = (parts + CT_SLICES - 1) / CT_SLICES;
    double s = 0.0, q = 0.0;
    for (int w = slice * per; w < (slice + 1) * per && w < parts; ++w) {
        s += partial[((size_t)w * 2 + 0) * D + c];
        q += partial[((size_t)w * 2 + 1) * D + c];
    }
    s = ct_combine(s, red, slice, c);
    q = ct_combine(q, red, slice, c);
    if (slice != 0) return;
    if (mode == 0) {
        const double mu = s / n;
        double var = q / n - mu * mu;
        var = var > 0.0 ? var : 0.0;
        const float muf = (float)mu, vf = (float)var;
        o0[c] = muf;
        o1[c] = vf;
        o2[c] = (float)(1.0 / sqrt(var + (double)cnn::BN_EPS));
        g0[c] = muf;
        g1[c] = vf;
    } else if (mode == 1) {
        o0[c] = (float)(s / n);
        o1[c] = (float)(q / n);
        g0[c] = beta_acc != 0.f ? fmaf(beta_acc, g0[c], (float)s) : (float)s;
        g1[c] = beta_acc != 0.f ? fmaf(beta_acc, g1[c], (float)q) : (float)q;
    } else {
        g0[c] = beta_acc != 0.f ? fmaf(beta_acc, g0[c], (float)s) : (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ BN, GELU, pool, choice, mask
// one thread per pooled element (b, j, c)
__global__ __launch_bounds__(256) void cnn_train_bnpool_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ g,
                                                               const float* __restrict__ beta, const unsigned char* __restrict__ keep,
                                                               float scale, float* __restrict__ xnext, unsigned char* __restrict__ choice,
                                                               int Lin, int Lout, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i & (D - 1));
    const size_t row = i >> 8, b = row / (size_t)Lout, j = row % (size_t)Lout;
    const float mu = mean[c], rs = rstd[c], gc = g[c], bc = beta[c];
    const float* zp = z + ((size_t)b * Lin + 4 * j) * D + c;
    float m = ct_y(zp[0], mu, rs, gc, bc);
    int ch = 0;
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float y = ct_y(zp[(size_t)r * D], mu, rs, gc, bc);
        if (y > m) {
            m = y;
            ch = r;
        }
    }
    if (keep) m = keep[i] ? m * scale : 0.f;
    xnext[i] = m;
    choice[i] = (unsigned char)ch;
}

// y on every position (clm_cnn_train_debug_fetch only)
__global__ __launch_bounds__(256) void cnn_train_y_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ g, const float* __restrict__ beta, float* __restrict__ y,
                                                          size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i & (D - 1));
    y[i] = ct_y(z[i], mean[c], rstd[c], g[c], beta[c]);
}

// pooled[b][c] = mean_j x[b][j][c]: four slices of j, each in order, in fp64
__global__ __launch_bounds__(1024) void cnn_train_mean_kernel(const float* __restrict__ x, int Lout, float* __restrict__ pooled) {
    __shared__ double red[CT_SLICES * D];
    const int b = blockIdx.x, c = threadIdx.x & (D - 1), slice = threadIdx.x >> 8, per = (Lout + CT_SLICES - 1) / CT_SLICES;
    const float* p = x + (size_t)b * Lout * D + c;
    double s = 0.0;
    for (int j = slice * per; j < (slice + 1) * per && j < Lout; ++j) s += (double)p[(size_t)j * D];
    s = ct_combine(s, red, slice, c);
    if (slice == 0) pooled[(size_t)b * D + c] = (float)(s / (double)Lout);
}

// ------------------------------------------------------------------------------------------------ backward, elementwise
// 256 threads (channel); workgroup w walks pooled rows [w chunk, (w + 1) chunk) of the B Lout: the gradient that reaches the pooled
// element (gin [B, Lout, 256], or dpooled[b] inv_l3 for block 2) through mask and scale to the chosen position, times gelu' there ->
// dyp; partial[w][0][c] = sum dy, [w][1][c] = sum dy xh
__global__ __launch_bounds__(256) void cnn_train_dy_kernel(const float* __restrict__ gin, const float* __restrict__ dpooled, float inv_l3,
                                                           const float* __restrict__ z, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ g,
                                                           const float* __restrict__ beta, const unsigned char* __restrict__ keep, float scale,
                                                           const unsigned char* __restrict__ choice, float* __restrict__ dyp,
                                                           double* __restrict__ partial, int Lin, int Lout, size_t rows, size_t chunk) {
    const int c = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    const float mu = mean[c], rs = rstd[c], gc = g[c], bc = beta[c];
    double s1 = 0.0, s2 = 0.0;
    for (size_t row = r0; row < r1; ++row) {
        const size_t b = row / (size_t)Lout, j = row % (size_t)Lout, i = row * D + c;
        float gi = gin ? gin[i] : dpooled[b * D + c] * inv_l3;
        if (keep) gi = keep[i] ? gi * scale : 0.f;
        const int r = choice[i];
        const float xh = (z[((size_t)b * Lin + 4 * j + r) * D + c] - mu) * rs;
        const float dy = gi * ct_gelu_grad(gc * xh + bc);
        dyp[i] = dy;
        s1 += (double)dy;
        s2 += (double)dy * (double)xh;
    }
    partial[((size_t)blockIdx.x * 2 + 0) * D + c] = s1;
    partial[((size_t)blockIdx.x * 2 + 1) * D + c] = s2;
}

// one thread per element (b, t, c): dz = g rstd (dy - m1 - xh m2), dy = dyp at the chosen position of a covered window, else 0
__global__ __launch_bounds__(256) void cnn_train_dz_kernel(const float* __restrict__ z, const float* __restrict__ dyp,
                                                           const unsigned char* __restrict__ choice, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ g,
                                                           const float* __restrict__ m1, const float* __restrict__ m2, float* __restrict__ dz,
                                                           int Lin, int Lout, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i & (D - 1));
    const size_t row = i >> 8, b = row / (size_t)Lin, t = row % (size_t)Lin, j = t >> 2;
    const float xh = (z[i] - mean[c]) * rstd[c];
    float dy = 0.f;
    if (j < (size_t)Lout) {
        const size_t pi = (b * Lout + j) * D + c;
        if (choice[pi] == (unsigned char)(t & 3)) dy = dyp[pi];
    }
    dz[i] = g[c] * rstd[c] * (dy - m1[c] - xh * m2[c]);
}

// ------------------------------------------------------------------------------------------------ dW, blocks 1 and 2
struct CnnTrainDwArgs {
    const float* dz;          // [B, Lin, 256]
    const float* x;           // [B, Lin, 256] the block's input
    float* partial;           // [gridDim.x][7][256 co][256 ci]
    int Lin, tiles_x, tiles;
};

// grid (G, 7 taps), 512 threads.  Per tile: the dz tile feature-major in Du (A operand), rows t0 + tap - 3 .. + 63 of x (zero outside
// the read) token-major in As (B operand), dacc[ct] += A . B over the tile's 64 tokens as pool_bwd_kernel does it
__global__ __launch_bounds__(512) void cnn_train_dw_kernel(CnnTrainDwArgs m) {
    extern __shared__ __attribute__((aligned(16))) float smem_ctw[];
    float* As = smem_ctw;                                   // [64][RS32]
    float* Du = As + BM32 * RS32;                           // [256][CT_RSD]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int Lin = m.Lin, tap = blockIdx.y;
    f32x16 dacc[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[ct][r] = 0.f;
    const int c0 = wave * 32 + 4 * lhalf;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < m.tiles; tile += gridDim.x) {
        const int b = tile / m.tiles_x, t0 = (tile % m.tiles_x) * BM32;
        {
            const float* src = m.x + (size_t)b * Lin * D + lane * 4;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = wave + 8 * i, t = t0 + tap - cnn::HALO + r;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (t >= 0 && t < Lin) v = *reinterpret_cast<const f32x4*>(src + (size_t)t * D);
                tile_store4<AR_F32>(As, r, lane * 4, v);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int t = t0 + mt * 32 + lrow;
            const bool ok = t < Lin;
            const float* row = m.dz + ((size_t)b * Lin + (ok ? t : Lin - 1)) * D + c0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 hv = *reinterpret_cast<const float4*>(row + 8 * q);
                float* d = Du + (c0 + 8 * q) * CT_RSD + mt * 32 + lrow;
                d[0] = ok ? hv.x : 0.f;
                d[CT_RSD] = ok ? hv.y : 0.f;
                d[2 * CT_RSD] = ok ? hv.z : 0.f;
                d[3 * CT_RSD] = ok ? hv.w : 0.f;
            }
        }
        __syncthreads();
        {
            const float* ap = Du + (wave * 32 + lrow) * CT_RSD + 8 * lhalf;
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
        __syncthreads();                                    // the next tile rewrites As and Du
    }
    {
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), lr = ln & 31, lh = ln >> 5;
        float* out = m.partial + ((size_t)blockIdx.x * cnn::K + tap) * D * D;
        float* orow = out + (size_t)(wave * 32 + 4 * lh) * D + lr;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) orow[acc_row(r, 0) * D + ct * 32] = dacc[ct][r];
    }
}

// dW[co][ci][tap] = beta dW + sum over the workgroups' partials, in workgroup order, in fp64
__global__ __launch_bounds__(256) void cnn_train_dw_reduce_kernel(const float* __restrict__ partial, int parts, float* __restrict__ dW, float beta) {
    const int i = blockIdx.x * 256 + threadIdx.x;              // < 7 * 65536
    const int tap = i / (D * D), rem = i % (D * D);
    double s = 0.0;
    for (int w = 0; w < parts; ++w) s += (double)partial[((size_t)w * cnn::K + tap) * D * D + rem];
    float* dst = dW + (size_t)rem * cnn::K + tap;
    *dst = beta != 0.f ? fmaf(beta, *dst, (float)s) : (float)s;
}

// ------------------------------------------------------------------------------------------------ block 0: dT, dW_0, dE
// 256 threads (channel co); workgroup w walks positions [w chunk, (w + 1) chunk) of the B L into its LDS table, CT_DT_SUB positions at a
// time: first the table row of every (position, tap) of the stretch into LDS (row 12: outside the read), then the walk
__global__ __launch_bounds__(256) void cnn_train_dt_kernel(const float* __restrict__ dz, const unsigned char* __restrict__ ids8, int Lp, int L,
                                                           size_t n, size_t chunk, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem_ctt[];   // [K][TROWS][256] | int [CT_DT_SUB][K]
    int* rowl = reinterpret_cast<int*>(smem_ctt + cnn::K * cnn::TROWS * D);
    const int c = threadIdx.x;
    for (int i = c; i < cnn::K * cnn::TROWS * D; i += 256) smem_ctt[i] = 0.f;
    float* Tc = smem_ctt + c;
    const size_t r0 = (size_t)blockIdx.x * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    for (size_t s0 = r0; s0 < r1; s0 += CT_DT_SUB) {
        const int cnt = (int)(r1 - s0 < (size_t)CT_DT_SUB ? r1 - s0 : (size_t)CT_DT_SUB);
        __syncthreads();                                               // the zeroed table; the walk before this stretch
        for (int i = c; i < cnt * cnn::K; i += 256) {
            const size_t r = s0 + i / cnn::K;
            const int dk = i % cnn::K, b = (int)(r / (size_t)L), tt = (int)(r % (size_t)L) + dk - cnn::HALO;
            int tok = cnn::VOC;
            if (tt >= 0 && tt < L) {
                tok = ids8[(size_t)b * Lp + tt];
                tok = tok < cnn::VOC ? tok : cnn::VOC - 1;
            }
            rowl[i] = (dk * cnn::TROWS + tok) * D;
        }
        __syncthreads();
        const float* src = dz + s0 * D + c;
        for (int i0 = 0; i0 < cnt; i0 += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = i0 + u < cnt ? src[(size_t)(i0 + u) * D] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u < cnt) {
                    const int* rw = rowl + (i0 + u) * cnn::K;
#pragma unroll
                    for (int dk = 0; dk < cnn::K; ++dk) Tc[rw[dk]] += v[u];
                }
            }
        }
    }
    float* out = partial + (size_t)blockIdx.x * CT_TSIZE;
    for (int dk = 0; dk < cnn::K; ++dk)
        for (int tok = 0; tok < cnn::VOC; ++tok) out[(dk * cnn::VOC + tok) * D + c] = Tc[(dk * cnn::TROWS + tok) * D];
}

// dT = the partials in workgroup order, as four slices of them, in fp64.  grid 7 x 12, 1,024 threads (co, slice)
__global__ __launch_bounds__(1024) void cnn_train_dt_reduce_kernel(const float* __restrict__ partial, int parts, float* __restrict__ dT) {
    __shared__ double red[CT_SLICES * D];
    const int c = threadIdx.x & (D - 1), slice = threadIdx.x >> 8, per = (parts + CT_SLICES - 1) / CT_SLICES, i = blockIdx.x * D + c;
    double s = 0.0;
    for (int w = slice * per; w < (slice + 1) * per && w < parts; ++w) s += (double)partial[(size_t)w * CT_TSIZE + i];
    s = ct_combine(s, red, slice, c);
    if (slice == 0) dT[i] = (float)s;
}

// grid 256 (co), 256 threads (ci): dW_0[co][ci][dk] = beta dW_0 + sum_tok dT[dk][tok][co] E[tok][ci]
__global__ __launch_bounds__(256) void cnn_train_dw0_kernel(const float* __restrict__ dT, const float* __restrict__ E, float* __restrict__ dW, float beta) {
    const int co = blockIdx.x, ci = threadIdx.x;
    float e[cnn::VOC];
#pragma unroll
    for (int tok = 0; tok < cnn::VOC; ++tok) e[tok] = E[tok * D + ci];
    for (int dk = 0; dk < cnn::K; ++dk) {
        double s = 0.0;
#pragma unroll
        for (int tok = 0; tok < cnn::VOC; ++tok) s += (double)dT[(dk * cnn::VOC + tok) * D + co] * (double)e[tok];
        float* dst = dW + ((size_t)co * D + ci) * cnn::K + dk;
        *dst = beta != 0.f ? fmaf(beta, *dst, (float)s) : (float)s;
    }
}

// grid 12 (tok), 1,024 threads (ci, slice of co): dE[tok][ci] = beta dE + sum_{co, dk} dT[dk][tok][co] W_0[co][ci][dk]; row 4
// (padding_idx): + 0
__global__ __launch_bounds__(1024) void cnn_train_de_kernel(const float* __restrict__ dT, const float* __restrict__ W, float* __restrict__ dE, float beta) {
    __shared__ double red[CT_SLICES * D];
    const int tok = blockIdx.x, ci = threadIdx.x & (D - 1), slice = threadIdx.x >> 8;
    double s = 0.0;
    if (tok != PAD_ID)
        for (int co = slice * (D / CT_SLICES); co < (slice + 1) * (D / CT_SLICES); ++co) {
            const float* w = W + ((size_t)co * D + ci) * cnn::K;
#pragma unroll
            for (int dk = 0; dk < cnn::K; ++dk) s += (double)dT[(dk * cnn::VOC + tok) * D + co] * (double)w[dk];
        }
    s = ct_combine(s, red, slice, ci);
    if (slice != 0) return;
    float* dst = dE + tok * D + ci;
    *dst = beta != 0.f ? fmaf(beta, *dst, (float)s) : (float)s;
}

}  // namespace clm

// ================================================================================================ engine + C ABI
using namespace clm;

struct clm_cnn_train_handle {
    int device = 0;
    std::string err;
    size_t limit = 0;                              // bytes of batch workspace a forward may take
    DevBuf ids8, z[3], dz[3], xn[3], choice[3], dyp, dx, part, fetch;
    DevBuf small;                                  // everything whose size does not depend on the batch (see Small)
    int B = 0, L = 0;
    int64_t gen = 0;                               // moves with every forward
    bool pending = false, have_dz = false, masked = false;
    float scale = 1.f;
    const unsigned char* keep[3] = {nullptr, nullptr, nullptr};
};

namespace {

constexpr size_t CT_DEFAULT_LIMIT = (size_t)64 << 30;
constexpr size_t CT_PART_BYTES = (size_t)CT_DW_GRID * cnn::K * D * D * 4;   // the largest of the three kinds of partials
static_assert(CT_PART_BYTES >= (size_t)CT_DT_GRID * CT_TSIZE * 4 && CT_PART_BYTES >= (size_t)CT_STAT_GRID * 2 * D * 8, "part holds every kind");

// offsets (floats) into `small`
struct Small {
    static constexpr size_t T = 0, DT = T + CT_TSIZE, E = DT + CT_TSIZE, W0 = E + cnn::VOC * D, MEAN = W0 + (size_t)D * D * cnn::K,
                            VAR = MEAN + 3 * D, RSTD = VAR + 3 * D, G = RSTD + 3 * D, BETA = G + 3 * D, M1 = BETA + 3 * D, M2 = M1 + D,
                            PACK = M2 + D,                                      // [block 1, 2][forward, flipped] x 7 x 65536
                            END = PACK + 4 * (size_t)cnn::K * D * D;
};

void ct_lens(int L, int (&Ls)[4]) {
    Ls[0] = L;
    for (int i = 0; i < 3; ++i) Ls[i + 1] = Ls[i] / 4;
}

// bytes of the batch's workspace: z, dz, x_{i+1}, choice, dyp per block, dx, ids
size_t ct_workspace_bytes(int B, int L) {
    int Ls[4];
    ct_lens(L, Ls);
    const size_t Lp = (size_t)(L + 63) / 64 * 64;
    size_t total = (size_t)B * Lp;
    for (int i = 0; i < 3; ++i) total += 2 * (size_t)B * Ls[i] * D * 4 + (size_t)B * Ls[i + 1] * D * 5;
    total += (size_t)B * Ls[1] * D * 4 * 2;        // dyp, dx: block 0's pooled size
    return total + CT_PART_BYTES;
}

void ct_split(size_t n, int max_grid, size_t min_chunk, size_t& chunk, int& grid) {
    size_t g = (n + min_chunk - 1) / min_chunk;
    if (g > (size_t)max_grid) g = max_grid;
    if (g < 1) g = 1;
    chunk = (n + g - 1) / g;
    grid = (int)((n + chunk - 1) / chunk);
}

void ct_gemm(const float* x, const float* w, const float* bias, float* out, int B, int Lin, hipStream_t st) {
    CnnTrainGemmArgs m{x, reinterpret_cast<const f32x4*>(w), bias, out, Lin, (Lin + BM32 - 1) / BM32};
    const size_t lds = (size_t)(BM32 + 2 * cnn::HALO) * RS32 * sizeof(float);
    launch_lds<cnn_train_gemm7_kernel>(dim3((unsigned)(m.tiles_x * B)), dim3(512), lds, st, m);
}

// column sums of v [n][256] -> `part`, then stats_final in `mode`
void ct_colsum(clm_cnn_train_handle* h, const float* v, size_t n, int mode, float* o0, float* o1, float* o2, float* g0, float* g1, float beta,
               hipStream_t st) {
    size_t chunk;
    int grid;
    ct_split(n, CT_STAT_GRID, 64, chunk, grid);
    hipLaunchKernelGGL(cnn_train_stats_kernel, dim3(grid), dim3(256), 0, st, v, n, chunk, h->part.get<double>());
    hipLaunchKernelGGL(cnn_train_stats_final_kernel, dim3(1), dim3(1024), 0, st, h->part.get<double>(), grid, (double)n, mode, o0, o1, o2, g0, g1,
                       beta);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int clm_cnn_train_create(int device, size_t workspace_limit_bytes, clm_cnn_train_handle** out) {
    if (!out) return fail<clm_cnn_train_handle>(nullptr, CLM_E_INVALID, "clm_cnn_train_create: bad argument");
    if (int rc = use_gfx950<clm_cnn_train_handle>(device, "clm_cnn_train_create")) return rc;
    clm_cnn_train_handle* h = new clm_cnn_train_handle();
    h->device = device;
    h->limit = workspace_limit_bytes ? workspace_limit_bytes : CT_DEFAULT_LIMIT;
    *out = h;
    return CLM_OK;
}

int64_t clm_cnn_train_generation(const clm_cnn_train_handle* h) { return h ? h->gen : -1; }

int clm_cnn_train_forward(clm_cnn_train_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L,
                          const float* const* params, const unsigned char* const* keep, float keep_scale, float* pooled_out,
                          float* mean_out, float* var_out, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!ids || !params || !pooled_out || !mean_out || !var_out || L < 1 || ids_row_stride < L)
        return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: bad argument");
    if (B < 2) return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: training needs a batch of at least 2 reads (batch statistics), got B = " + std::to_string(B));
    if (B > 65535) return fail(h, CLM_E_UNSUPPORTED, "clm_cnn_train_forward: at most 65535 reads in a batch (a grid dimension), got B = " + std::to_string(B));
    if (L < 64)
        return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: DNAConvNet needs reads of at least 64 tokens (three max-pools of 4), got L = " + std::to_string(L));
    if (ids_dtype != CLM_DT_I64 && ids_dtype != CLM_DT_I32 && ids_dtype != CLM_DT_U8)
        return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: ids dtype must be i64, i32 or u8");
    for (int i = 0; i < CLM_CNN_TRAIN_PARAMS; ++i)
        if (!params[i] || !aligned16(params[i])) return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: parameter " + std::to_string(i) + " is null or not 16-byte aligned");
    if ((size_t)B * (size_t)L > ((size_t)1 << 30)) return fail(h, CLM_E_UNSUPPORTED, "clm_cnn_train_forward: more than 2^30 tokens in a batch");
    const size_t need = ct_workspace_bytes(B, L);
    if (need > h->limit)
        return fail(h, CLM_E_INVALID, "clm_cnn_train_forward: a batch of " + std::to_string(B) + " x " + std::to_string(L) + " tokens needs " +
                                          std::to_string(need) + " bytes of workspace, the limit is " + std::to_string(h->limit) +
                                          " bytes; BatchNorm couples the reads of a batch, so it is not computed in pieces");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    h->pending = false;
    h->have_dz = false;
    ++h->gen;
    int Ls[4];
    ct_lens(L, Ls);
    const int Lp = (L + 63) / 64 * 64;
    if (int rc = grow(h, Sync::Device(), {
            {&h->ids8, (size_t)B * Lp},
            {&h->z[0], (size_t)B * Ls[0] * D * 4}, {&h->z[1], (size_t)B * Ls[1] * D * 4}, {&h->z[2], (size_t)B * Ls[2] * D * 4},
            {&h->dz[0], (size_t)B * Ls[0] * D * 4}, {&h->dz[1], (size_t)B * Ls[1] * D * 4}, {&h->dz[2], (size_t)B * Ls[2] * D * 4},
            {&h->xn[0], (size_t)B * Ls[1] * D * 4}, {&h->xn[1], (size_t)B * Ls[2] * D * 4}, {&h->xn[2], (size_t)B * Ls[3] * D * 4},
            {&h->choice[0], (size_t)B * Ls[1] * D}, {&h->choice[1], (size_t)B * Ls[2] * D}, {&h->choice[2], (size_t)B * Ls[3] * D},
            {&h->dyp, (size_t)B * Ls[1] * D * 4}, {&h->dx, (size_t)B * Ls[1] * D * 4}, {&h->part, CT_PART_BYTES}, {&h->small, Small::END * 4}}))
        return rc;
    float* const sm = h->small.get<float>();
    const float* E = params[0];
    const float *W[3], *bias[3], *g[3], *beta[3];
    for (int i = 0; i < 3; ++i) W[i] = params[1 + 4 * i], bias[i] = params[2 + 4 * i], g[i] = params[3 + 4 * i], beta[i] = params[4 + 4 * i];
    // what the backward reads of the parameters: the forward's own copies
    HIPCHK(h, hipMemcpyAsync(sm + Small::E, E, (size_t)cnn::VOC * D * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(sm + Small::W0, W[0], (size_t)D * D * cnn::K * 4, hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < 3; ++i) {
        HIPCHK(h, hipMemcpyAsync(sm + Small::G + i * D, g[i], D * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(sm + Small::BETA + i * D, beta[i], D * 4, hipMemcpyDeviceToDevice, st));
    }
    for (int i = 1; i < 3; ++i)
        for (int flip = 0; flip < 2; ++flip)
            hipLaunchKernelGGL(cnn_train_pack_kernel, dim3(cnn::K * D * D / 4 / 256), dim3(256), 0, st, W[i],
                               reinterpret_cast<f32x4*>(sm + Small::PACK + (size_t)(2 * (i - 1) + flip) * cnn::K * D * D), flip);
    unsigned char* const ids8 = h->ids8.get<unsigned char>();
    launch_embed(ids, ids_dtype, ids_row_stride, nullptr, nullptr, ids8, B, L, Lp, st);
    hipLaunchKernelGGL(cnn_train_table_kernel, dim3(cnn::K * cnn::VOC), dim3(1024), 0, st, E, W[0], sm + Small::T);
    {
        const size_t lds = (size_t)cnn::K * cnn::TROWS * D * 4 + (size_t)(CT_PT0 + 2 * cnn::HALO) * 4;
        launch_lds<cnn_train_conv0_kernel>(dim3((unsigned)((L + CT_PT0 - 1) / CT_PT0), (unsigned)B), dim3(512), lds, st, ids8, Lp, sm + Small::T,
                                           bias[0], h->z[0].get<float>(), L);
    }
    h->masked = keep != nullptr;
    h->scale = keep_scale;
    for (int i = 0; i < 3; ++i) {
        const int Lin = Ls[i], Lout = Ls[i + 1];
        float* const z = h->z[i].get<float>();
        if (i > 0) ct_gemm(h->xn[i - 1].get<float>(), sm + Small::PACK + (size_t)(2 * (i - 1)) * cnn::K * D * D, bias[i], z, B, Lin, st);
        ct_colsum(h, z, (size_t)B * Lin, 0, sm + Small::MEAN + i * D, sm + Small::VAR + i * D, sm + Small::RSTD + i * D, mean_out + i * D,
                  var_out + i * D, 0.f, st);
        h->keep[i] = keep ? keep[i] : nullptr;
        const size_t total = (size_t)B * Lout * D;
        hipLaunchKernelGGL(cnn_train_bnpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z, sm + Small::MEAN + i * D,
                           sm + Small::RSTD + i * D, sm + Small::G + i * D, sm + Small::BETA + i * D, h->keep[i], keep_scale,
                           h->xn[i].get<float>(), h->choice[i].get<unsigned char>(), Lin, Lout, total);
    }
    hipLaunchKernelGGL(cnn_train_mean_kernel, dim3(B), dim3(1024), 0, st, h->xn[2].get<float>(), Ls[3], pooled_out);
    h->B = B;
    h->L = L;
    if (int rc = launched(h, "clm_cnn_train_forward")) return rc;
    h->pending = true;
    return CLM_OK;
}

int clm_cnn_train_backward(clm_cnn_train_handle* h, int64_t generation, const float* dpooled, float* const* grads, float beta, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!dpooled || !grads || (beta != 0.f && beta != 1.f)) return fail(h, CLM_E_INVALID, "clm_cnn_train_backward: bad argument (beta is 0 or 1)");
    for (int i = 0; i < CLM_CNN_TRAIN_PARAMS; ++i)
        if (!grads[i]) return fail(h, CLM_E_INVALID, "clm_cnn_train_backward: gradient " + std::to_string(i) + " is null");
    if (!h->pending) return fail(h, CLM_E_STATE, "clm_cnn_train_backward: no forward is pending on this handle");
    if (generation != h->gen)
        return fail(h, CLM_E_STATE, "clm_cnn_train_backward: another forward ran on this handle since the one to differentiate; its "
                                    "intermediates are gone");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int B = h->B, L = h->L, Lp = (L + 63) / 64 * 64;
    int Ls[4];
    ct_lens(L, Ls);
    float* const sm = h->small.get<float>();
    float* const dyp = h->dyp.get<float>();
    float* const dx = h->dx.get<float>();
    for (int i = 2; i >= 0; --i) {
        const int Lin = Ls[i], Lout = Ls[i + 1];
        float *dW = grads[1 + 4 * i], *db = grads[2 + 4 * i], *dg = grads[3 + 4 * i], *dbeta = grads[4 + 4 * i];
        const float *z = h->z[i].get<float>(), *mean = sm + Small::MEAN + i * D, *rstd = sm + Small::RSTD + i * D, *g = sm + Small::G + i * D,
                    *bt = sm + Small::BETA + i * D;
        float* const dz = h->dz[i].get<float>();
        const unsigned char* ch = h->choice[i].get<unsigned char>();
        {
            size_t chunk;
            int grid;
            const size_t rows = (size_t)B * Lout;
            ct_split(rows, CT_STAT_GRID, 16, chunk, grid);
            hipLaunchKernelGGL(cnn_train_dy_kernel, dim3(grid), dim3(256), 0, st, i == 2 ? nullptr : dx, dpooled, 1.0f / (float)Ls[3], z, mean, rstd, g,
                               bt, h->masked ? h->keep[i] : nullptr, h->scale, ch, dyp, h->part.get<double>(), Lin, Lout, rows, chunk);
            hipLaunchKernelGGL(cnn_train_stats_final_kernel, dim3(1), dim3(1024), 0, st, h->part.get<double>(), grid, (double)((size_t)B * Lin), 1,
                               sm + Small::M1, sm + Small::M2, (float*)nullptr, dbeta, dg, beta);
        }
        const size_t total = (size_t)B * Lin * D;
        hipLaunchKernelGGL(cnn_train_dz_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z, dyp, ch, mean, rstd, g, sm + Small::M1,
                           sm + Small::M2, dz, Lin, Lout, total);
        ct_colsum(h, dz, (size_t)B * Lin, 2, nullptr, nullptr, nullptr, db, nullptr, beta, st);
        if (i > 0) {
            ct_gemm(dz, sm + Small::PACK + (size_t)(2 * (i - 1) + 1) * cnn::K * D * D, nullptr, dx, B, Lin, st);   // dx_i [B, L_i, 256]
            const int tiles_x = (Lin + BM32 - 1) / BM32, tiles = tiles_x * B, grid = tiles < CT_DW_GRID ? tiles : CT_DW_GRID;
            CnnTrainDwArgs m{dz, h->xn[i - 1].get<float>(), h->part.get<float>(), Lin, tiles_x, tiles};
            const size_t lds = (size_t)(BM32 * RS32 + D * CT_RSD) * sizeof(float);
            launch_lds<cnn_train_dw_kernel>(dim3((unsigned)grid, cnn::K), dim3(512), lds, st, m);
            hipLaunchKernelGGL(cnn_train_dw_reduce_kernel, dim3(cnn::K * D * D / 256), dim3(256), 0, st, h->part.get<float>(), grid, dW, beta);
        } else {
            size_t chunk;
            int grid;
            const size_t n = (size_t)B * L;
            ct_split(n, CT_DT_GRID, 128, chunk, grid);
            launch_lds<cnn_train_dt_kernel>(dim3((unsigned)grid), dim3(256), (size_t)cnn::K * cnn::TROWS * D * 4 + (size_t)CT_DT_SUB * cnn::K * 4, st, dz, h->ids8.get<unsigned char>(), Lp,
                                            L, n, chunk, h->part.get<float>());
            hipLaunchKernelGGL(cnn_train_dt_reduce_kernel, dim3(cnn::K * cnn::VOC), dim3(1024), 0, st, h->part.get<float>(), grid, sm + Small::DT);
            hipLaunchKernelGGL(cnn_train_dw0_kernel, dim3(D), dim3(256), 0, st, sm + Small::DT, sm + Small::E, dW, beta);
            hipLaunchKernelGGL(cnn_train_de_kernel, dim3(cnn::VOC), dim3(1024), 0, st, sm + Small::DT, sm + Small::W0, grads[0], beta);
        }
    }
    h->pending = false;
    if (int rc = launched(h, "clm_cnn_train_backward")) return rc;
    h->have_dz = true;
    return CLM_OK;
}

int clm_cnn_train_debug_fetch(clm_cnn_train_handle* h, const char* name, void* host_out, size_t bytes) {
    if (!h || !name || !host_out) return fail(h, CLM_E_INVALID, "clm_cnn_train_debug_fetch: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const std::string n(name);
    if (h->B < 1) return fail(h, CLM_E_STATE, "clm_cnn_train_debug_fetch before a forward");
    int Ls[4];
    ct_lens(h->L, Ls);
    const int i = n.empty() ? -1 : n.back() - '0';
    const std::string stem = n.empty() ? n : n.substr(0, n.size() - 1);
    if (i < 0 || i > 2 || (stem != "z" && stem != "y" && stem != "choice" && stem != "dz"))
        return fail(h, CLM_E_INVALID, "clm_cnn_train_debug_fetch: unknown name " + n + " (z0..z2, y0..y2, choice0..choice2, dz0..dz2)");
    const size_t full = (size_t)h->B * Ls[i] * D * 4, pooled = (size_t)h->B * Ls[i + 1] * D;
    const void* src = nullptr;
    size_t have = full;
    if (stem == "z") src = h->z[i].get();
    else if (stem == "choice") { src = h->choice[i].get(); have = pooled; }
    else if (stem == "dz") {
        if (!h->have_dz) return fail(h, CLM_E_STATE, "clm_cnn_train_debug_fetch: dz exists after clm_cnn_train_backward");
        src = h->dz[i].get();
    } else {
        float* const sm = h->small.get<float>();
        HIPCHK(h, h->fetch.reserve(full));
        const size_t total = full / 4;
        hipLaunchKernelGGL(cnn_train_y_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, h->z[i].get<float>(), sm + Small::MEAN + i * D,
                           sm + Small::RSTD + i * D, sm + Small::G + i * D, sm + Small::BETA + i * D, h->fetch.get<float>(), total);
        HIPCHK(h, hipDeviceSynchronize());
        src = h->fetch.get();
    }
    return fetch_bytes(h, "clm_cnn_train_debug_fetch", n, src, have, host_out, bytes);
}

int64_t clm_cnn_train_workspace_bytes(int B, int L) { return B < 1 || L < 64 ? (int64_t)CLM_E_INVALID : (int64_t)ct_workspace_bytes(B, L); }

const char* clm_cnn_train_last_error(const clm_cnn_train_handle* h) {
    return h ? h->err.c_str() : create_error<clm_cnn_train_handle>().c_str();
}

int clm_cnn_train_destroy(clm_cnn_train_handle* h) { return destroy_handle(h); }

}  // extern "C"
