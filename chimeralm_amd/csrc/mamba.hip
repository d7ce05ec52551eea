// mamba.hip -- the reference's two Mamba2 classifiers on MI355X: kernels + engine + C ABI (clm_mamba_*).
//
// Reference: the reference's chimeralm/models/components/mamba.py, configs/model/mamba.yaml (MambaSequenceClassification: d 256,
// 12 layers, d_state 16 / 64, expand 2, a learned positional term, Linear + LayerNorm in front, an optional mask) and
// configs/model/mambasp.yaml (MambaSequenceClassificationSP: d 512, 3 layers, d_state 128, expand 3, the embedding alone), both
// around mamba_ssm.Mamba2 with its defaults (tests/mamba_reference.py states the arithmetic once):
//   [z | xBC | dt] = in_proj(h);  xBC = silu(causal depthwise conv, 4 taps) -> x | B | C;  dt = softplus(dt + dt_bias)
//   S_t = exp(dt_t A) S_{t-1} + dt_t B_t x_t^T,  y_t = C_t^T S_t + D x_t            (per head: N x 64 state, A = -exp(A_log))
//   h += out_proj(norm.weight * g * rsqrt(mean(g^2) + 1e-5)),  g = y * silu(z)       (then * mask, `mamba` only)
//   pooled = (mean_t h + max_t h) / 2 ;  Linear + GELU ;  Linear + GELU + Linear -> 2 logits
//
// Launches per chunk of reads (the engine bounds its workspace by running long batches in chunks of whole reads):
//   front     mamba: mamba_proj_kernel<EPI_FRONT> (E[id] + pos gathered into the tile, Linear) + mamba_front_ln_kernel (LayerNorm,
//             mask); mambasp: mamba_embed_kernel (E[id])
//   per layer mamba_proj_kernel<EPI_INPROJ>: in_proj on the MFMA (exact fp32 or fp16x3), softplus(dt + dt_bias) in the epilogue
//             mamba_conv_kernel: the causal depthwise conv + SiLU of x | B | C, once per token (B and C are shared by all heads)
//             mamba_scan_kernel<N>: one workgroup walks one (read, head) through its 64-token chunks: the chunk's cumulative decay,
//             the intra-chunk and state products on the fp32 MFMA, the D skip, g = y * silu(z), and per-(token, head) sums of
//             squares of g.  Exact fp32 in both precisions.
//             mamba_proj_kernel<EPI_OUT / EPI_OUTPOOL>: out_proj with norm.weight folded into its columns (fp64, at finalize); the
//             epilogue reduces the heads' sums of squares in a fixed order (the RMSNorm spans all heads), scales, adds the
//             residual, applies the mask; the last layer writes per-64-row-tile channel sums and maxima instead of the rows.
//   head      mamba_head_kernel<d>: the tiles' partials in a fixed order, pooler, classifier.
// No atomics: the forward is bitwise deterministic and a read's logits do not depend on its batch-mates.
// The constants, silu / softplus, ScanShape, the conv + SiLU body, the decay scan and the head's dense layer are mamba_common.h's,
// shared with mamba_train.hip and mamba_verdict.hip.
// clm_mamba_debug_fetch also reads the workspace itself -- "zx", "xc", "g", "ssq", "part": the LAST layer's in_proj output, conv
// output, scan output, per-head sums of squares and pooling partials -- after a forward that ran as one chunk of reads.
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "chimeralm_hip.h"
#include "handle_host.h"
#include "mamba_common.h"
#include "mfma32_common.h"

namespace clm {
namespace mamba {

using namespace ssm;               // P, Q, DCONV, EPS, silu, softplus, ScanShape and the device routines shared with training (mamba_common.h)
constexpr int VOC = 12;
constexpr float X3_RANGE = 65504.f;   // fp16x3 splits an activation exactly only below fp16's largest finite value

enum { EPI_FRONT = 0, EPI_INPROJ = 1, EPI_OUT = 2, EPI_OUTPOOL = 3 };

// ------------------------------------------------------------------------------------------------ projections
// out[row][c] = sum_k W[c][k] A[row][k] on 64-token tiles x 256 output features (8 waves x 32), K in chunks of 256 staged in LDS and
// multiplied by mfma32_common.h's product256 (the weight-set pipeline of tail32.hip).  Row = b * L + t; rows t >= L stage as zero and
// are not written.  Grid: (reads x tiles_x) x nblocks, the 256-wide output block fastest.
struct ProjArgs {
    const float* a;                 // A [rows][lda]                                   (EPI_FRONT: unused)
    int lda;
    const unsigned char* ids8;      // EPI_FRONT: A row (b, t) = emb[ids8[b Lp + t]] + pos[t]
    int Lp;
    const float *emb, *pos;
    const f32x4* w;                 // packed [nblocks][8 waves][K / 8][64 lanes] (launch_pack_f32t / launch_pack_x3)
    int K;                          // multiple of 256
    float* out;                     // [rows][ldo]; EPI_OUT*: the residual stream, updated in place
    int ldo;
    const float* bias;              // EPI_FRONT: [ldo]; EPI_INPROJ: dt_bias [H]
    int dt0, H;                     // EPI_INPROJ: columns dt0 .. dt0 + H - 1 are dt; EPI_OUT*: heads per row of ssq
    const float* ssq;               // EPI_OUT*: [rows][H] per-head sums of squares of g
    float inv_di;                   // 1 / d_inner
    const float* mask;              // EPI_OUT*: [reads][mask_stride] or null
    int64_t mask_stride;
    float* part;                    // EPI_OUTPOOL: [reads][tiles_x][2][ldo] channel sums | maxima of the tile's rows
    int store;                      // EPI_OUTPOOL: also write the rows (debug taps of a one-layer net)
    int n_real;                     // output columns that carry weights: the waves whose 32 columns all lie beyond it (in_proj's zero
                                    // padding to a multiple of 256) skip their products
    int L, tiles_x, nblocks;
};

template <int EPI, int AR>
__global__ __launch_bounds__(512) void mamba_proj_kernel(ProjArgs m) {
    constexpr float WSI = WUNSCALE<AR>;
    extern __shared__ __attribute__((aligned(16))) float smem_mp[];
    float* Xs = smem_mp;                                    // [64][RS32] A tile (fp32, or hi | lo halfs)
    __shared__ int saturated;                               // fp16x3: an activation beyond fp16's range was staged
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int nb = (int)blockIdx.x % m.nblocks, tg = (int)blockIdx.x / m.nblocks;
    const int b = tg / m.tiles_x, tile = tg % m.tiles_x, t0 = tile * BM32, L = m.L;
    const int ksteps = m.K / 8, kchunks = m.K / 256;
    const bool live = nb * 256 + wave * 32 < m.n_real;     // (wave-uniform)
    if (tid == 0) saturated = 0;
    f32x4 ws[2][KS_SET];
    f32x16 acc[2];
    if (live) load_wset(wset_ptr(m.w, nb, ksteps, 0, wave, lane), ws[0]);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    bool big = false;
    for (int kc = 0; kc < kchunks; ++kc) {
        __syncthreads();                                    // (the previous chunk's product has read Xs; `saturated` is set)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave + 8 * i, t = t0 + r, col = kc * 256 + lane * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < L) {
                if constexpr (EPI == EPI_FRONT) {
                    int id = m.ids8[(size_t)b * m.Lp + t];
                    id = id < VOC ? id : VOC - 1;
                    v = *reinterpret_cast<const f32x4*>(m.emb + (size_t)id * m.K + col) +
                        *reinterpret_cast<const f32x4*>(m.pos + (size_t)t * m.K + col);
                } else {
                    v = *reinterpret_cast<const f32x4*>(m.a + ((size_t)b * L + t) * m.lda + col);
                }
            }
            if constexpr (AR == AR_X3) {
#pragma unroll
                for (int e = 0; e < 4; ++e) big |= !(fabsf(v[e]) <= X3_RANGE);
            }
            tile_store4<AR>(Xs, r, lane * 4, v);
        }
        __syncthreads();
        const f32x4* nxt = wset_ptr(m.w, nb, ksteps, kc + 1 < kchunks ? (kc + 1) * 4 * KS_SET : 0, wave, lane);
        if (live) product256<false, AR>(Xs, m.w, nb, ksteps, kc * 4 * KS_SET, nxt, wave, lane, ws, acc);
    }
    // fp16x3 cannot represent an activation beyond fp16's range (the split saturates): the tile's outputs become NaN, so the
    // caller sees a non-finite logit and reruns the batch on the exact-fp32 kernels (chimeralm_amd/mamba.py)
    bool poison = false;
    if constexpr (AR == AR_X3) {
        if (big) saturated = 1;                             // (every writer stores the same value)
        __syncthreads();
        poison = saturated != 0;
    }
    const int cbase = nb * 256 + wave * 32 + 4 * lhalf;
    float psum[4][4], pmax[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) psum[q][e] = 0.f, pmax[q][e] = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int t = t0 + mt * 32 + lrow;
        const bool valid = t < L;
        const size_t row = (size_t)b * L + (valid ? t : 0);
        float rms = 0.f, mk = 1.f;
        if constexpr (EPI == EPI_OUT || EPI == EPI_OUTPOOL) {
            if (valid) {
                float s = 0.f;
                for (int hh = 0; hh < m.H; ++hh) s += m.ssq[row * m.H + hh];
                rms = rsqrtf(s * m.inv_di + EPS);
                if (m.mask) mk = m.mask[(size_t)b * m.mask_stride + t];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = cbase + 8 * q;
            float* o = m.out + row * m.ldo + c;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = poison ? __builtin_nanf("") : acc[mt][4 * q + e] * WSI;
            if constexpr (EPI == EPI_FRONT) {
                v += *reinterpret_cast<const f32x4*>(m.bias + c);
            } else if constexpr (EPI == EPI_INPROJ) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e >= m.dt0 && c + e < m.dt0 + m.H) v[e] = softplus(v[e] + m.bias[c + e - m.dt0]);
            } else {
                if (valid) {
                    const f32x4 hv = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (hv[e] + v[e] * rms) * mk;
                }
            }
            if constexpr (EPI == EPI_OUTPOOL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    psum[q][e] += valid ? v[e] : 0.f;
                    pmax[q][e] = valid ? fmaxf(pmax[q][e], v[e]) : pmax[q][e];
                }
                if (valid && m.store) *reinterpret_cast<f32x4*>(o) = v;
            } else {
                if (valid) *reinterpret_cast<f32x4*>(o) = v;
            }
        }
    }
    if constexpr (EPI == EPI_OUTPOOL) {
        // the 32 rows of each half-wave in a fixed butterfly; lane 0 / 32 writes its four features x 4
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = psum[q][e], x = pmax[q][e];
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {
                    s += __shfl_xor(s, o, 64);
                    x = fmaxf(x, __shfl_xor(x, o, 64));
                }
                psum[q][e] = s, pmax[q][e] = x;
            }
        if (lrow == 0) {
            float* po = m.part + ((size_t)b * m.tiles_x + tile) * 2 * m.ldo + cbase;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                *reinterpret_cast<float4*>(po + 8 * q) = make_float4(psum[q][0], psum[q][1], psum[q][2], psum[q][3]);
                *reinterpret_cast<float4*>(po + m.ldo + 8 * q) = make_float4(pmax[q][0], pmax[q][1], pmax[q][2], pmax[q][3]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ front
// mamba: LayerNorm (two-pass statistics) of the Linear's rows, then the mask; one wave per row of DV x 64 features
template <int DV>
__global__ __launch_bounds__(256) void mamba_front_ln_kernel(const float* __restrict__ y, const float* __restrict__ gam,
                                                             const float* __restrict__ bet, const float* __restrict__ mask,
                                                             int64_t mask_stride, float* __restrict__ h, int rows, int L) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)rows) return;
    constexpr int d = DV * 64;
    float v[DV], s = 0.f;
#pragma unroll
    for (int k = 0; k < DV; ++k) s += (v[k] = y[row * d + lane + 64 * k]);
    const float mean = wave_sum(s) * (1.0f / d);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < DV; ++k) q += (v[k] - mean) * (v[k] - mean);
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / d) + EPS);
    const float mk = mask ? mask[(row / L) * mask_stride + row % L] : 1.f;
#pragma unroll
    for (int k = 0; k < DV; ++k) {
        const int c = lane + 64 * k;
        h[row * d + c] = ((v[k] - mean) * rstd * gam[c] + bet[c]) * mk;
    }
}

// mambasp: h = E[id]; one wave per row
__global__ __launch_bounds__(256) void mamba_embed_kernel(const unsigned char* __restrict__ ids8, int Lp, const float* __restrict__ emb,
                                                          float* __restrict__ h, int rows, int L, int d) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)rows) return;
    int id = ids8[(row / L) * Lp + row % L];
    id = id < VOC ? id : VOC - 1;
    for (int c = lane; c < d; c += 64) h[row * d + c] = emb[(size_t)id * d + c];
}

// ------------------------------------------------------------------------------------------------ conv
// The causal depthwise conv + SiLU of all conv_dim columns (x | B | C), once per token: xc[row][c] = silu(b[c] + sum_k w[c][k]
// zx[row - 3 + k][di + c]), rows before the read's start counting as zero.  Four channels per thread.
__global__ __launch_bounds__(256) void mamba_conv_kernel(const float* __restrict__ zx, int ldz, int di, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ xc, int conv_dim, int rows,
                                                         int L) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per_row = (size_t)conv_dim / 4;
    if (i >= (size_t)rows * per_row) return;
    const size_t row = i / per_row;
    conv4_silu(zx, ldz, di, w, bias, xc, conv_dim, row, (int)(row % L), 4 * (int)(i % per_row));
}

// ------------------------------------------------------------------------------------------------ scan
// One workgroup (4 waves) per (read, head), walking the read's 64-token chunks in order.  Per chunk, with s_i = sum_{k <= i} dt_k A:
//   G^T[j][i] = (B_j . C_i) exp(s_i - s_j) dt_j for j <= i, exactly 0 above the diagonal (never exp of a positive difference)
//   y^T = exp(s_i) S^T C^T + X^T G^T ;  y += D x ;  g = y * silu(z) ;  sum over the head's 64 channels of g^2
//   S = exp(s_63) S + (w B)^T X,  w_j = exp(s_63 - s_j) dt_j          (s_63: dt = 0 past the read)
// All four products on v_mfma_f32_32x32x2_f32 (exact fp32).  Wave (pi, mi) owns the 32 x 32 output tile (channels p in
// [32 pi, 32 pi + 32), tokens i in [32 mi, 32 mi + 32)) of y^T and the N x 32 state columns of its p range, in accumulator layout
// (so the state is the A operand of S^T C^T without leaving registers; the two waves of one p range keep identical copies).  Its
// G^T tiles stay in registers too: their accumulator layout is the B operand X^T G^T reads.  x rows come from xc straight into
// registers in operand layout; only B and C (rows of N + 1 floats: conflict-free column reads) and the decay terms sit in LDS --
// 67 KB at N = 128, two workgroups per CU.  N < 32 is padded to 32 with zero columns.
struct ScanArgs {
    const float* xc;                // [rows][ldx] conv + SiLU output: x | B | C
    int ldx;
    const float* zx;                // [rows][ldz] in_proj output: z in columns [0, di), dt (softplus applied) in column dt0 + h
    int ldz, dt0;
    const float *A_log, *Dp;        // [H]
    float *g, *ssq;                 // [rows][di], [rows][H]
    int L, di, H;
};

template <int N>
constexpr size_t scan_lds_floats = (size_t)2 * Q * ScanShape<N>::BS + 4 * Q + 2 * Q + 4;   // B, C, sv | es | wj | dts, Rs, eL

template <int N>
__global__ __launch_bounds__(256, 2) void mamba_scan_kernel(ScanArgs m) {   // (two workgroups per CU: <= 256 registers)
    using SH = ScanShape<N>;
    constexpr int NP = SH::NP, NT = SH::NT, BS = SH::BS;
    extern __shared__ __attribute__((aligned(16))) float smem_ms[];
    float* Bs = smem_ms;                                    // [Q][BS]
    float* Cs = Bs + Q * BS;                                // [Q][BS]
    float* sv = Cs + Q * BS;                                // [Q] s_i
    float* es = sv + Q;                                     // [Q] exp(s_i)
    float* wj = es + Q;                                     // [Q] exp(s_63 - s_j) dt_j
    float* dts = wj + Q;                                    // [Q] dt
    float* Rs = dts + Q;                                    // [2][Q] sums of g^2 over each 32-channel half
    float* eL = Rs + 2 * Q;                                 // [1] exp(s_63)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int pi = wave & 1, mi = wave >> 1, p0 = 32 * pi, i0 = 32 * mi;
    const int h = (int)blockIdx.x % m.H, b = (int)blockIdx.x / m.H, L = m.L, di = m.di, hP = h * P;
    const float A = -expf(m.A_log[h]), Dh = m.Dp[h];
    const float* xr_base = m.xc + (size_t)b * L * m.ldx;
    const float* zr = m.zx + (size_t)b * L * m.ldz;
    for (int k = tid; k < Q * (BS - N); k += 256) {          // the padding columns stay zero
        const int i = k / (BS - N), n = N + k % (BS - N);
        Bs[i * BS + n] = 0.f;
        Cs[i * BS + n] = 0.f;
    }
    f32x16 S[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) S[nt][r] = 0.f;
    const int nch = (L + Q - 1) / Q;
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * Q;
        // ---- B, C rows -> LDS; dt; this wave's x operand straight to registers: xo[jt][4 q + e] = x[32 jt + 8 q + 4 lhalf + e][p0 + lrow]
        for (int k = tid; k < Q * N; k += 256) {
            const int i = k / N, n = k % N, t = c0 + i;
            const float* src = xr_base + (size_t)t * m.ldx + di + n;
            Bs[i * BS + n] = t < L ? src[0] : 0.f;
            Cs[i * BS + n] = t < L ? src[N] : 0.f;
        }
        if (tid < Q) dts[tid] = c0 + tid < L ? zr[(size_t)(c0 + tid) * m.ldz + m.dt0 + h] : 0.f;
        float xo[2][16];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = c0 + 32 * jt + acc_row(r, lhalf);
                xo[jt][r] = t < L ? xr_base[(size_t)t * m.ldx + hP + p0 + lrow] : 0.f;
            }
        __syncthreads();
        if (wave == 0) {                                    // cumulative decay: a fixed-order wave scan
            float a, last;
            decay_scan(lane, dts[lane] * A, a, last);
            sv[lane] = a;
            es[lane] = expf(a);
            wj[lane] = expf(last - a) * dts[lane];
            if (lane == 0) eL[0] = expf(last);
        }
        __syncthreads();
        // ---- y^T tile: X^T G^T, one G^T tile (j rows, i = i0 + lrow columns) at a time for j-tiles 0 .. mi (above: all zero) ...
        const int icol = i0 + lrow;
        const float si = sv[icol];
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.f;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
            if (jt <= mi) {
                f32x16 Gt;
#pragma unroll
                for (int r = 0; r < 16; ++r) Gt[r] = 0.f;
                const float* ba = Bs + (32 * jt + lrow) * BS + lhalf;
                const float* cb = Cs + icol * BS + lhalf;
#pragma unroll 2
                for (int s = 0; s < NP / 2; ++s) Gt = mfma32(ba[2 * s], cb[2 * s], Gt);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * jt + acc_row(r, lhalf);
                    const bool keep = j <= icol;
                    const float e = expf(keep ? si - sv[j] : 0.f);
                    Gt[r] = keep ? Gt[r] * e * dts[j] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) y = mfma32(xo[jt][r], Gt[r], y);
                __builtin_amdgcn_sched_barrier(0);
            }
        // ... + exp(s_i) S^T C^T
        {
            f32x16 yi;
#pragma unroll
            for (int r = 0; r < 16; ++r) yi[r] = 0.f;
            const float* cb = Cs + icol * BS + 4 * lhalf;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) yi = mfma32(S[nt][r], cb[32 * nt + acc_row(r, 0)], yi);
                __builtin_amdgcn_sched_barrier(0);          // (bounds what the scheduler hoists: registers, not spills)
            }
            const float ei = es[icol];
#pragma unroll
            for (int r = 0; r < 16; ++r) y[r] += ei * yi[r];
        }
        // ---- epilogue: element (p = p0 + 8 q + 4 lhalf + e, i = icol) in y[4 q + e]
        {
            const int t = c0 + icol;
            float ss = 0.f;
            if (t < L) {
                const size_t row = (size_t)b * L + t;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p = hP + p0 + 8 * q + 4 * lhalf;
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr_base + (size_t)t * m.ldx + p);
                    const f32x4 zv = *reinterpret_cast<const f32x4*>(zr + (size_t)t * m.ldz + p);
                    f32x4 gv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        gv[e] = (y[4 * q + e] + Dh * xv[e]) * silu(zv[e]);
                        ss += gv[e] * gv[e];
                    }
                    *reinterpret_cast<f32x4*>(m.g + row * di + p) = gv;
                }
            }
            ss += __shfl_xor(ss, 32, 64);
            if (lhalf == 0) Rs[pi * Q + icol] = ss;
        }
        // ---- state: S = exp(s_63) S + (w B)^T X over this wave's p columns
        {
            const float e63 = eL[0];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) S[nt][r] *= e63;
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = 32 * jt + acc_row(r, lhalf);
                        S[nt] = mfma32(Bs[j * BS + 32 * nt + lrow] * wj[j], xo[jt][r], S[nt]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();                                    // Rs complete; Bs / Cs / decay terms free for the next chunk
        if (tid < Q && c0 + tid < L) m.ssq[((size_t)b * L + c0 + tid) * m.H + h] = Rs[tid] + Rs[Q + tid];
    }
}

// ------------------------------------------------------------------------------------------------ head
// one workgroup per read: the tiles' sums and maxima in a fixed order, pooled = (mean + max) / 2, pooler (Linear + GELU), classifier
// (Linear + GELU + Linear); DV = d threads; the d-wide layers (weights transposed at finalize: coalesced) are head_dense on one row
template <int DV>
__global__ __launch_bounds__(DV) void mamba_head_kernel(const float* __restrict__ part, int tiles, int L, const float* __restrict__ wpt,
                                                        const float* __restrict__ bp, const float* __restrict__ w0t, const float* __restrict__ b0,
                                                        const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ pooled,
                                                        float* __restrict__ logits) {
    constexpr int D2 = DV / 2;
    __shared__ __attribute__((aligned(16))) float Pv[1][DV];
    __shared__ __attribute__((aligned(16))) float X1[1][DV];
    __shared__ __attribute__((aligned(16))) float X2[1][D2];
    const int tid = threadIdx.x, b = blockIdx.x;
    {
        const float* src = part + (size_t)b * tiles * 2 * DV + tid;
        float s = 0.f, mx = -INFINITY;
        for (int i = 0; i < tiles; ++i) {
            s += src[(size_t)i * 2 * DV];
            mx = fmaxf(mx, src[(size_t)i * 2 * DV + DV]);
        }
        const float v = (s / (float)L + mx) * 0.5f;
        Pv[0][tid] = v;
        pooled[(size_t)b * DV + tid] = v;
    }
    __syncthreads();
    float a;
    head_dense<1, DV>(wpt, DV, tid, bp[tid], Pv, &a);                          // pooler.0 + GELU
    X1[0][tid] = gelu_erf(a);
    __syncthreads();
    if (tid < D2) {
        head_dense<1, DV>(w0t, D2, tid, b0[tid], X1, &a);                      // classifier.0 + GELU
        X2[0][tid] = gelu_erf(a);
    }
    __syncthreads();
    if (tid < NCLS) {                                                          // classifier.3: the bias last
        a = 0.f;
        for (int c = 0; c < D2; ++c) a = fmaf(w3[(size_t)tid * D2 + c], X2[0][c], a);
        logits[(size_t)b * NCLS + tid] = a + b3[tid];
    }
}

template <int EPI>
void launch_proj(const ProjArgs& m, int reads, bool x3, hipStream_t st) {
    const dim3 grid((unsigned)((size_t)reads * m.tiles_x * m.nblocks)), block(512);
    const size_t lds = (size_t)BM32 * RS32 * sizeof(float);
    if (x3) launch_lds<mamba_proj_kernel<EPI, AR_X3>>(grid, block, lds, st, m);
    else launch_lds<mamba_proj_kernel<EPI, AR_F32>>(grid, block, lds, st, m);
}

void launch_scan(const ScanArgs& m, int N, int reads, hipStream_t st) {
    const dim3 grid((unsigned)((size_t)m.H * reads)), block(256);            // (read, head) -> blockIdx.x = read * H + head
    switch (N) {
        case 16: launch_lds<mamba_scan_kernel<16>>(grid, block, scan_lds_floats<16> * 4, st, m); break;
        case 32: launch_lds<mamba_scan_kernel<32>>(grid, block, scan_lds_floats<32> * 4, st, m); break;
        case 64: launch_lds<mamba_scan_kernel<64>>(grid, block, scan_lds_floats<64> * 4, st, m); break;
        default: launch_lds<mamba_scan_kernel<128>>(grid, block, scan_lds_floats<128> * 4, st, m); break;
    }
}

}  // namespace mamba
}  // namespace clm

// ================================================================================================ engine + C ABI
using namespace clm;

// Weights as the kernels take them: device pointers resolved ONCE, by clm_mamba_finalize, and the packings it makes
struct MambaLayer {               // one Mamba2 layer
    DevBuf in, out;               // in_proj (rows padded to n_in_pad), out_proj with norm.weight folded in: packed for the MFMA (f32t, or x3 halfs)
    const float *dt_bias, *A_log, *D, *conv_w, *conv_b;   // as loaded, fp32
};
struct MambaNetF32 {              // ... and what belongs to no layer, as loaded: embedding, the front block (CLM_MAMBA_SEQ), head biases, classifier.3
    const float *emb, *pos, *front_b, *front_ln_g, *front_ln_b, *pool_b, *cls0_b, *cls3_w, *cls3_b;
};

struct clm_mamba_handle {
    int device = 0;
    int variant = 0;                              // CLM_MAMBA_SEQ (mamba) or CLM_MAMBA_SP (mambasp)
    int d = 0, n_layers = 0, N = 0, expand = 0, max_len = 0;
    int di = 0, H = 0, conv_dim = 0, n_in = 0, n_in_pad = 0;
    bool x3 = false, x3_active = false;
    std::string err;
    std::map<std::string, DevBuf> w;              // fp32 device copies by reference key
    WeightTable expected;                         // (clm_mamba_create)
    std::vector<MambaLayer> layer;                // [n_layers], sized by clm_mamba_create: `expected` points into it
    MambaNetF32 net = {};
    DevBuf front, poolert, cls0t;                 // finalize products: input_block.0 packed; pooler.0 / classifier.0 weights transposed
    bool finalized = false;
    DevBuf ids8, h, zx, xc, g, ssq, part, pooled, dbg_front, dbg_layer0;   // workspace (clm_mamba_forward)
    DevBuf verdict_pooled, verdict_npad;          // the running verdict (mamba_verdict.hip): fp32 [chunk reads][K][d], int [chunk reads]; grown by the first request
    int last_B = 0, last_L = 0, last_nb = 0;     // ... and the reads per chunk of the last forward
    bool last_dbg = false;
};

namespace {

constexpr size_t ZX_CAP = size_t(4) << 30;        // bytes of in_proj output per chunk of reads (the largest workspace buffer)
constexpr size_t DBG_CAP = size_t(256) << 20;     // "front" / "layer0" taps are kept up to this many bytes each

std::string layer_prefix(const clm_mamba_handle* h, int i) {
    return "mamba_layers." + std::to_string(i) + (h->variant == CLM_MAMBA_SEQ ? ".mamba." : ".");
}

// clm_mamba_create: the state-dict keys, their shapes and the field of h->net / h->layer the forward reads each from (none: finalize's)
void mamba_expect(clm_mamba_handle* h) {
    WeightTable& e = h->expected;
    MambaNetF32& n = h->net;
    const int64_t d = h->d;
    h->layer.resize(h->n_layers);
    e["embedding.weight"] = {{mamba::VOC, d}, &n.emb};
    if (h->variant == CLM_MAMBA_SEQ) {
        e["pos_embedding"] = {{1, h->max_len, d}, &n.pos};
        e["input_block.0.weight"] = {{d, d}, nullptr}; e["input_block.0.bias"] = {{d}, &n.front_b};
        e["input_block.1.weight"] = {{d}, &n.front_ln_g}; e["input_block.1.bias"] = {{d}, &n.front_ln_b};
    }
    for (int i = 0; i < h->n_layers; ++i) {
        const std::string p = layer_prefix(h, i);
        MambaLayer& l = h->layer[i];
        e[p + "in_proj.weight"] = {{h->n_in, d}, nullptr};
        e[p + "conv1d.weight"] = {{h->conv_dim, 1, ssm::DCONV}, &l.conv_w}; e[p + "conv1d.bias"] = {{h->conv_dim}, &l.conv_b};
        e[p + "dt_bias"] = {{h->H}, &l.dt_bias}; e[p + "A_log"] = {{h->H}, &l.A_log}; e[p + "D"] = {{h->H}, &l.D};
        e[p + "norm.weight"] = {{h->di}, nullptr}; e[p + "out_proj.weight"] = {{d, h->di}, nullptr};
    }
    e["pooler.0.weight"] = {{d, d}, nullptr}; e["pooler.0.bias"] = {{d}, &n.pool_b};
    e["classifier.0.weight"] = {{d / 2, d}, nullptr}; e["classifier.0.bias"] = {{d / 2}, &n.cls0_b};
    e["classifier.3.weight"] = {{NCLS, d / 2}, &n.cls3_w}; e["classifier.3.bias"] = {{NCLS}, &n.cls3_b};
}

int mamba_host(clm_mamba_handle* h, const std::string& k, std::vector<float>& out) { return host_f32(h, "clm_mamba_finalize", k, out); }

// W [rows][K] (rows <= rows_pad, zero rows appended) -> the MFMA packing of the handle's arithmetic
int mamba_pack(clm_mamba_handle* h, DevBuf& dst, const std::vector<float>& W, int rows, int rows_pad, int K) {
    std::vector<float> padded((size_t)rows_pad * K, 0.f);
    std::copy(W.begin(), W.begin() + (size_t)rows * K, padded.begin());
    DevBuf src, q;
    if (int rc = upload_f32(h, src, padded)) return rc;
    HIPCHK(h, q.alloc(padded.size() * 4));
    if (h->x3_active) launch_pack_x3(src.get<float>(), q.get(), rows_pad, K, 0);
    else launch_pack_f32t(src.get<float>(), q.get(), rows_pad, K, 0);
    HIPCHK(h, hipDeviceSynchronize());                 // (`src` is freed on return)
    dst = std::move(q);
    return CLM_OK;
}

}  // namespace

extern "C" {

int clm_mamba_create(int device, int variant, int precision, int d_model, int n_layers, int d_state, int expand, int headdim,
                     int model_max_length, clm_mamba_handle** out) {
    if (!out) return fail<clm_mamba_handle>(nullptr, CLM_E_INVALID, "clm_mamba_create: bad argument");
    if (variant != CLM_MAMBA_SEQ && variant != CLM_MAMBA_SP)
        return fail<clm_mamba_handle>(nullptr, CLM_E_INVALID, "clm_mamba_create: variant must be CLM_MAMBA_SEQ or CLM_MAMBA_SP");
    if (precision != CLM_PREC_F32 && precision != CLM_PREC_F16X3)
        return fail<clm_mamba_handle>(nullptr, CLM_E_INVALID, "clm_mamba_create: precision must be CLM_PREC_F32 (exact) or CLM_PREC_F16X3");
    const bool ok = (d_model == 256 || d_model == 512) && n_layers >= 1 && (d_state == 16 || d_state == 32 || d_state == 64 || d_state == 128) &&
                    expand >= 1 && (expand * d_model) % 64 == 0 && headdim == ssm::P && (variant == CLM_MAMBA_SP || model_max_length >= 1);
    if (!ok)
        return fail<clm_mamba_handle>(nullptr, CLM_E_INVALID, "clm_mamba_create: supported shapes are d_model 256 or 512, at least one layer, "
                                                              "d_state 16 / 32 / 64 / 128, headdim 64, expand >= 1 (and model_max_length >= 1 "
                                                              "for CLM_MAMBA_SEQ)");
    if (int rc = use_gfx950<clm_mamba_handle>(device, "clm_mamba_create")) return rc;
    clm_mamba_handle* h = new clm_mamba_handle();
    h->device = device;
    h->variant = variant;
    h->x3 = precision == CLM_PREC_F16X3;
    h->d = d_model, h->n_layers = n_layers, h->N = d_state, h->expand = expand;
    h->max_len = variant == CLM_MAMBA_SEQ ? model_max_length : 0;
    h->di = expand * d_model;
    h->H = h->di / ssm::P;
    h->conv_dim = h->di + 2 * d_state;
    h->n_in = 2 * h->di + 2 * d_state + h->H;
    h->n_in_pad = (h->n_in + 255) / 256 * 256;
    mamba_expect(h);
    *out = h;
    return CLM_OK;
}

int clm_mamba_load_weight(clm_mamba_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !key || !data || !shape || ndim < 0) return fail(h, CLM_E_INVALID, "clm_mamba_load_weight: null argument");
    const std::string k = canonical_weight_key(key);
    if (dtype != CLM_DT_F32) return fail(h, CLM_E_INVALID, "clm_mamba_load_weight: fp32 tensors only");
    return load_f32(h, "clm_mamba_load_weight", k, data, shape, ndim);
}

int clm_mamba_finalize(clm_mamba_handle* h) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = resolve_weights(h, "clm_mamba_finalize")) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    for (MambaLayer& l : h->layer) l.in.reset(), l.out.reset();
    for (DevBuf* b : {&h->front, &h->poolert, &h->cls0t}) b->reset();
    h->finalized = false;
    int rc;
    const int d = h->d, di = h->di;
    // the projections as the MFMA reads them; out_proj with norm.weight folded into its columns in fp64.  fp16x3 packs w x 2^10 as
    // fp16 hi + lo, which saturates for |w| >= 64: such weights run in the exact-fp32 packing (chimeralm_amd/mamba.py reports it)
    std::vector<std::vector<float>> win(h->n_layers), wout(h->n_layers);
    std::vector<float> wfront;
    float wmax = 0.f;
    auto track = [&](const std::vector<float>& v) {
        for (float x : v) wmax = std::fmax(wmax, std::fabs(x));
    };
    for (int i = 0; i < h->n_layers; ++i) {
        const std::string p = layer_prefix(h, i);
        std::vector<float> nw;
        if ((rc = mamba_host(h, p + "in_proj.weight", win[i])) || (rc = mamba_host(h, p + "out_proj.weight", wout[i])) ||
            (rc = mamba_host(h, p + "norm.weight", nw)))
            return rc;
        for (int c = 0; c < d; ++c)
            for (int k = 0; k < di; ++k) wout[i][(size_t)c * di + k] = (float)((double)wout[i][(size_t)c * di + k] * (double)nw[k]);
        track(win[i]);
        track(wout[i]);
    }
    if (h->variant == CLM_MAMBA_SEQ) {
        if ((rc = mamba_host(h, "input_block.0.weight", wfront))) return rc;
        track(wfront);
    }
    h->x3_active = h->x3 && wmax < X3_WEIGHT_LIMIT;
    for (int i = 0; i < h->n_layers; ++i) {
        if ((rc = mamba_pack(h, h->layer[i].in, win[i], h->n_in, h->n_in_pad, d))) return rc;
        if ((rc = mamba_pack(h, h->layer[i].out, wout[i], d, d, di))) return rc;
    }
    if (h->variant == CLM_MAMBA_SEQ && (rc = mamba_pack(h, h->front, wfront, d, d, d))) return rc;
    {
        std::vector<float> wp, w0;
        if ((rc = mamba_host(h, "pooler.0.weight", wp)) || (rc = mamba_host(h, "classifier.0.weight", w0))) return rc;
        if ((rc = upload_f32(h, h->poolert, transposed(wp, d, d))) || (rc = upload_f32(h, h->cls0t, transposed(w0, d / 2, d)))) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    return CLM_OK;
}

int clm_mamba_forward(clm_mamba_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, const float* mask,
                      int64_t mask_row_stride, float* logits_out, void* stream) {
    return clm_mamba_forward_traj(h, ids, ids_dtype, ids_row_stride, B, L, mask, mask_row_stride, logits_out, nullptr, stream);
}

int clm_mamba_forward_traj(clm_mamba_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, const float* mask,
                           int64_t mask_row_stride, float* logits_out, const clm_traj_out* traj, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_mamba_forward before clm_mamba_finalize");
    if (int rc = check_ids_arg(h, "clm_mamba_forward", ids, logits_out, ids_dtype, ids_row_stride, B, L)) return rc;
    if (h->variant == CLM_MAMBA_SEQ && L > h->max_len)
        return fail(h, CLM_E_INVALID, "clm_mamba_forward: read length " + std::to_string(L) + " exceeds model_max_length " +
                                          std::to_string(h->max_len) + " (the positional embedding's length)");
    if (mask && mask_row_stride < L) return fail(h, CLM_E_INVALID, "clm_mamba_forward: mask row stride shorter than the read");
    if (int rc = check_traj_request(h, "clm_mamba_forward_traj", traj, L)) return rc;
    if (h->variant == CLM_MAMBA_SP) mask = nullptr;              // (the reference's mambasp ignores its second argument)
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int d = h->d, di = h->di, H = h->H, N = h->N, NP = h->n_in_pad, Lp = (L + 63) / 64 * 64, tiles_x = (L + 63) / 64;
    const size_t cap_tok = ZX_CAP / ((size_t)NP * 4);
    const int nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, cap_tok / (size_t)L));
    const size_t T = (size_t)nb * L;
    const bool dbg = (size_t)B * L * d * 4 <= DBG_CAP;
    const size_t taps = dbg ? (size_t)B * L * d * 4 : 0;
    const int vK = traj ? (L + traj->stride - 1) / traj->stride : 0;          // points per read of the request
    if (int rc = grow(h, Sync::Device(), {{&h->ids8, (size_t)B * Lp}, {&h->h, T * d * 4}, {&h->zx, T * NP * 4}, {&h->xc, T * h->conv_dim * 4},
                                          {&h->g, T * di * 4}, {&h->ssq, T * H * 4}, {&h->part, (size_t)nb * tiles_x * 2 * d * 4},
                                          {&h->pooled, (size_t)B * d * 4}, {&h->dbg_front, taps}, {&h->dbg_layer0, taps},
                                          {&h->verdict_pooled, (size_t)nb * vK * d * 4}, {&h->verdict_npad, traj ? (size_t)nb * 4 : 0}}))
        return rc;
    const MambaNetF32& net = h->net;
    unsigned char* const ids8 = h->ids8.get<unsigned char>();
    float *const hs = h->h.get<float>(), *const zx = h->zx.get<float>(), *const g = h->g.get<float>(), *const ssq = h->ssq.get<float>();
    launch_embed(ids, ids_dtype, ids_row_stride, nullptr, nullptr, ids8, B, L, Lp, st);   // ids of any dtype -> clamped bytes
    const bool x3 = h->x3_active;
    for (int r0 = 0; r0 < B; r0 += nb) {
        const int n = std::min(nb, B - r0), rows = n * L;
        const float* mk = mask ? mask + (size_t)r0 * mask_row_stride : nullptr;
        const unsigned char* id8 = ids8 + (size_t)r0 * Lp;
        const unsigned row_blocks = (unsigned)(((size_t)rows + 3) / 4);
        if (h->variant == CLM_MAMBA_SEQ) {
            mamba::ProjArgs f{};
            f.ids8 = id8, f.Lp = Lp, f.emb = net.emb, f.pos = net.pos, f.w = h->front.get<f32x4>(), f.K = d;
            f.out = zx, f.ldo = d, f.bias = net.front_b, f.L = L, f.tiles_x = tiles_x, f.nblocks = d / 256, f.n_real = d;
            mamba::launch_proj<mamba::EPI_FRONT>(f, n, x3, st);
            hipLaunchKernelGGL(d == 256 ? mamba::mamba_front_ln_kernel<4> : mamba::mamba_front_ln_kernel<8>, dim3(row_blocks), dim3(256), 0, st,
                               zx, net.front_ln_g, net.front_ln_b, mk, mask_row_stride, hs, rows, L);
        } else {
            hipLaunchKernelGGL(mamba::mamba_embed_kernel, dim3(row_blocks), dim3(256), 0, st, id8, Lp, net.emb, hs, rows, L, d);
        }
        if (dbg)
            HIPCHK(h, hipMemcpyAsync(h->dbg_front.get<float>() + (size_t)r0 * L * d, hs, (size_t)rows * d * 4, hipMemcpyDeviceToDevice, st));
        for (int l = 0; l < h->n_layers; ++l) {
            const MambaLayer& ly = h->layer[l];
            const bool last = l + 1 == h->n_layers;
            mamba::ProjArgs a{};
            a.a = hs, a.lda = d, a.w = ly.in.get<f32x4>(), a.K = d, a.out = zx, a.ldo = NP, a.bias = ly.dt_bias;
            a.dt0 = 2 * di + 2 * N, a.H = H, a.L = L, a.tiles_x = tiles_x, a.nblocks = NP / 256, a.n_real = h->n_in;
            mamba::launch_proj<mamba::EPI_INPROJ>(a, n, x3, st);
            {
                const size_t quads = (size_t)rows * h->conv_dim / 4;
                hipLaunchKernelGGL(mamba::mamba_conv_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, zx, NP, di,
                                   ly.conv_w, ly.conv_b, h->xc.get<float>(), h->conv_dim, rows, L);
            }
            mamba::ScanArgs s{h->xc.get<float>(), h->conv_dim, zx, NP, 2 * di + 2 * N, ly.A_log, ly.D, g, ssq, L, di, H};
            mamba::launch_scan(s, N, n, st);
            mamba::ProjArgs o{};
            o.a = g, o.lda = di, o.w = ly.out.get<f32x4>(), o.K = di, o.out = hs, o.ldo = d, o.H = H, o.ssq = ssq;
            o.inv_di = 1.0f / (float)di, o.mask = mk, o.mask_stride = mask_row_stride, o.part = h->part.get<float>();
            o.store = dbg && l == 0, o.L = L, o.tiles_x = tiles_x, o.nblocks = d / 256, o.n_real = d;
            if (last) mamba::launch_proj<mamba::EPI_OUTPOOL>(o, n, x3, st);
            else mamba::launch_proj<mamba::EPI_OUT>(o, n, x3, st);
            if (dbg && l == 0)
                HIPCHK(h, hipMemcpyAsync(h->dbg_layer0.get<float>() + (size_t)r0 * L * d, hs, (size_t)rows * d * 4, hipMemcpyDeviceToDevice, st));
        }
        hipLaunchKernelGGL(d == 256 ? mamba::mamba_head_kernel<256> : mamba::mamba_head_kernel<512>, dim3((unsigned)n), dim3(d), 0, st,
                           h->part.get<float>(), tiles_x, L, h->poolert.get<float>(), net.pool_b, h->cls0t.get<float>(), net.cls0_b, net.cls3_w,
                           net.cls3_b, h->pooled.get<float>() + (size_t)r0 * d, logits_out + (size_t)r0 * NCLS);
        if (traj) {
            // the chunk's running verdict at the rows of its reads in the caller's buffers: the prefix pooling of the partials the
            // forward left, pooler and classifier over the interior points, then the chunk's own logits into the last point and the
            // summary (mamba_verdict.hip, trajectory.hip)
            float* const out = traj->logits + (size_t)r0 * traj->point_stride * NCLS;
            int* const npad = h->verdict_npad.get<int>();
            launch_ssm_verdict_pool(h->part.get<float>(), tiles_x, traj->stride / 64, vK, L, d, h->verdict_pooled.get<float>(), id8, Lp,
                                    npad, n, st);
            launch_ssm_verdict_head(h->verdict_pooled.get<float>(), vK, n * (vK - 1), d, h->poolert.get<float>(), net.pool_b,
                                    h->cls0t.get<float>(), net.cls0_b, net.cls3_w, net.cls3_b, out, traj->point_stride, st);
            launch_traj_summary(logits_out + (size_t)r0 * NCLS, out, traj->point_stride, n, vK, traj->stride, L, npad, id8, Lp,
                                traj->summary ? traj->summary + r0 : nullptr, st);
        }
    }
    h->last_B = B, h->last_L = L, h->last_nb = nb, h->last_dbg = dbg;
    return launched(h, "clm_mamba_forward");
}

int clm_mamba_debug_fetch(clm_mamba_handle* h, const char* name, void* host_out, size_t bytes) {
    if (!h || !name || !host_out) return fail(h, CLM_E_INVALID, "clm_mamba_debug_fetch: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const std::string n(name);
    const size_t B = (size_t)h->last_B, L = (size_t)h->last_L, d = (size_t)h->d;
    const void* src = nullptr;
    size_t have = 0;
    if (n == "front" || n == "layer0") {
        if (!h->last_dbg) return fail(h, CLM_E_INVALID, "clm_mamba_debug_fetch: the last forward was too large to keep " + n);
        src = n == "front" ? h->dbg_front.get() : h->dbg_layer0.get();
        have = B * L * d * 4;
    } else if (n == "pooled") {
        src = h->pooled.get();
        have = B * d * 4;
    } else if (n == "zx" || n == "xc" || n == "g" || n == "ssq" || n == "part") {
        // the workspace as the last layer of the last chunk of reads left it: the whole batch only when it ran as one chunk
        if (h->last_nb < h->last_B)
            return fail(h, CLM_E_INVALID, "clm_mamba_debug_fetch: the last forward ran in chunks of " + std::to_string(h->last_nb) +
                                              " reads; " + n + " holds the last chunk only");
        const size_t T = B * L;
        if (n == "zx") src = h->zx.get(), have = T * (size_t)h->n_in_pad * 4;
        else if (n == "xc") src = h->xc.get(), have = T * (size_t)h->conv_dim * 4;
        else if (n == "g") src = h->g.get(), have = T * (size_t)h->di * 4;
        else if (n == "ssq") src = h->ssq.get(), have = T * (size_t)h->H * 4;
        else src = h->part.get(), have = B * ((L + 63) / 64) * 2 * d * 4;
    } else {
        return fail(h, CLM_E_INVALID, "clm_mamba_debug_fetch: unknown name " + n);
    }
    return fetch_bytes(h, "clm_mamba_debug_fetch", n, src, have, host_out, bytes);
}

const char* clm_mamba_last_error(const clm_mamba_handle* h) { return h ? h->err.c_str() : create_error<clm_mamba_handle>().c_str(); }

int clm_mamba_destroy(clm_mamba_handle* h) { return destroy_handle(h); }

}  // extern "C"
