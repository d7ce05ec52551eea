// mamba_train.hip -- the core of one Mamba2 layer in training form, forward and backward, behind clm_mamba_train_* (DESIGN.md 5.13).
//
// The core is what lies between in_proj and out_proj (tests/mamba_reference.py, tests/mamba_train_reference.py):
//   zxbcdt [B, L, 2 di + 2 N + H] = z | xBC | dt   ->   xc = silu(causal depthwise conv, 4 taps, + bias) = x | B | C ;
//   dt = softplus(raw + dt_bias) ;  ys = scan(x, dt, A, B, C) + D x ;  g = ys silu(z) ;  out = norm.weight g rsqrt(mean_c g^2 + 1e-5)
// Exact fp32; every matrix product on v_mfma_f32_32x32x2_f32; no floating-point atomics, every reduction in a fixed order, partials
// of different workgroups combined in fp64 in workgroup order (mtrain_reduce_kernel): the same inputs give the same bits.
//
// Forward launches:   mtrain_pre_kernel (conv + SiLU, softplus), mtrain_scan_fwd_kernel<N> (one workgroup per (read, head) walks the
//                     64-token chunks, leaving ys and every chunk's ENTRY state), mtrain_gate_fwd_kernel (gate + RMSNorm, a wave per row)
// Backward launches:  mtrain_gate_bwd_kernel (dys, dz, partials of d norm.weight per 64 rows),
//                     mtrain_scan_bwd_kernel<N> (one workgroup per (read, head) walks the chunks in REVERSE carrying dS: dx, ddt, this
//                     head's dB | dC, its dA_log and dD),
//                     mtrain_conv_bwd_kernel (sums dB | dC over the heads in head order, SiLU and the four taps backwards inside the
//                     read, partials of d conv1d.weight / bias per 64-token tile), mtrain_dt_bwd_kernel (softplus backwards, partials
//                     of d dt_bias), mtrain_reduce_kernel x 6.
// Both scan kernels keep their operands in LDS (rows of 64 + 1 or N + 1 floats: row-wise and column-wise operand reads are both
// conflict-free) and their 32 x 32 output tiles in the MFMA accumulators; the carried state (S forward, dS backward) lives in LDS
// too and is updated in place, a tile at a time, by the wave that owns the tile.
// What the inference kernels state alike -- constants, silu / softplus, ScanShape, the conv + SiLU body, the decay scan -- is
// mamba_common.h's; acc_row is clm_common.h's.
#include <algorithm>
#include <string>

#include "chimeralm_hip.h"
#include "handle_host.h"
#include "mamba_common.h"
#include "mfma32_common.h"

namespace clm {
namespace mtrain {

using namespace ssm;               // P, Q, DCONV, EPS, silu, softplus, ScanShape and the device routines shared with inference (mamba_common.h)
constexpr int XS = Q + 1;          // row stride (floats) of the 64-wide LDS tiles

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float dsilu(float v) {
    const float s = sigm(v);
    return s * (1.0f + v * (1.0f - s));
}

// sum over the 32 lanes of a half-wave in a fixed butterfly (every lane of the half receives it)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// LDS bytes of the two scans: X, G (backward: + dys), B, C, the state, the vectors
template <int N, int NP = ScanShape<N>::NP, int BS = ScanShape<N>::BS>
constexpr size_t fwd_lds = ((size_t)2 * Q * XS + 2 * Q * BS + NP * XS + 4 * Q + 4) * 4;
template <int N, int NP = ScanShape<N>::NP, int BS = ScanShape<N>::BS>
constexpr size_t bwd_lds = ((size_t)3 * Q * XS + 2 * Q * BS + NP * XS + 4 * Q + 6 * Q + 2 * 4 * Q + 2 * 256 + 4) * 4;

// ------------------------------------------------------------------------------------------------ forward
// xc[row][c] = silu(b[c] + sum_k w[c][k] xBC[row - 3 + k][c]) inside the read (four channels per thread), dt[row][h] = softplus(raw + dt_bias)
__global__ __launch_bounds__(256) void mtrain_pre_kernel(const float* __restrict__ zx, int ldz, int di, int conv_dim, int H,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ dt_bias, float* __restrict__ xc, float* __restrict__ dt,
                                                         size_t rows, int L) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per_row = (size_t)conv_dim / 4 + H;
    if (i >= rows * per_row) return;
    const size_t row = i / per_row;
    const int k4 = (int)(i % per_row);
    if (k4 >= conv_dim / 4) {
        const int h = k4 - conv_dim / 4;
        dt[row * H + h] = softplus(zx[row * ldz + di + conv_dim + h] + dt_bias[h]);
        return;
    }
    conv4_silu(zx, ldz, di, w, bias, xc, conv_dim, row, (int)(row % L), 4 * k4);
}

struct ScanArgs {
    const float* xc;                // [rows][ldx] x | B | C
    int ldx;
    const float* dt;                // [rows][H]
    const float *A_log, *Dp;        // [H]
    float* ys;                      // forward: out [rows][di] = y + D x
    float* states;                  // [B][H][nch][N][P] chunk entry states (forward: written; backward: read)
    const float* dys;               // backward: [rows][di]
    float *dx, *ddt, *dbc;          // backward: [rows][di], [rows][H], [B][H][L][2 N] (this head's dB | dC)
    float *pA, *pD;                 // backward: [B][H] dA_log and dD of one (read, head)
    int L, di, H, nch;
};

// chunk loads shared by both scans: rows of the read past L stage as zeros (dt = 0: no decay, no input)
template <int N>
__device__ __forceinline__ void load_chunk(const ScanArgs& m, int b, int h, int c0, int tid, float* Xs, float* Bs, float* Cs, float* dts) {
    constexpr int BS = ScanShape<N>::BS;
    const float* xr = m.xc + (size_t)b * m.L * m.ldx;
    for (int k = tid; k < Q * P; k += 256) {
        const int i = k / P, p = k % P, t = c0 + i;
        Xs[i * XS + p] = t < m.L ? xr[(size_t)t * m.ldx + h * P + p] : 0.f;
    }
    for (int k = tid; k < Q * N; k += 256) {
        const int i = k / N, n = k % N, t = c0 + i;
        const float* src = xr + (size_t)t * m.ldx + m.di + n;
        Bs[i * BS + n] = t < m.L ? src[0] : 0.f;
        Cs[i * BS + n] = t < m.L ? src[N] : 0.f;
    }
    if (tid < Q) dts[tid] = c0 + tid < m.L ? m.dt[((size_t)b * m.L + c0 + tid) * m.H + h] : 0.f;
}

// s_i = sum_{k <= i} dt_k A (wave 0; decay_scan): sv = s, es = exp(s), fs = exp(s_63 - s_j), eL = exp(s_63)
__device__ __forceinline__ void chunk_decay(int lane, float A, const float* dts, float* sv, float* es, float* fs, float* eL) {
    float a, last;
    decay_scan(lane, dts[lane] * A, a, last);
    sv[lane] = a;
    es[lane] = expf(a);
    fs[lane] = expf(last - a);
    if (lane == 0) eL[0] = expf(last);
}

// One workgroup (4 waves) per (read, head).  Per chunk: G_ij = (C_i . B_j) exp(s_i - s_j) dt_j for j <= i, exactly 0 above the diagonal
// (only non-positive differences are exponentiated); ys = G X + exp(s_i) C S + D x; S = exp(s_63) S + (f dt B)^T X.
template <int N>
__global__ __launch_bounds__(256) void mtrain_scan_fwd_kernel(ScanArgs m) {
    using SH = ScanShape<N>;
    constexpr int NP = SH::NP, NT = SH::NT, BS = SH::BS;
    extern __shared__ __attribute__((aligned(16))) float smem_mt[];
    float* Xs = smem_mt;                 // [Q][XS]
    float* Gs = Xs + Q * XS;             // [Q][XS]
    float* Bs = Gs + Q * XS;             // [Q][BS]
    float* Cs = Bs + Q * BS;             // [Q][BS]
    float* Ss = Cs + Q * BS;             // [NP][XS] the state, n-major
    float* sv = Ss + NP * XS;
    float* es = sv + Q;
    float* fs = es + Q;
    float* dts = fs + Q;
    float* eL = dts + Q;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int h = (int)blockIdx.x % m.H, b = (int)blockIdx.x / m.H, L = m.L;
    const float A = -expf(m.A_log[h]), Dh = m.Dp[h];
    for (int k = tid; k < 2 * Q * BS + NP * XS; k += 256) Bs[k] = 0.f;      // B, C padding columns and the zero initial state
    const int it = wave >> 1, jt = wave & 1;                                 // this wave's 32 x 32 tile of a 64 x 64 output
    for (int ch = 0; ch < m.nch; ++ch) {
        const int c0 = ch * Q;
        __syncthreads();                                                     // the previous chunk's state is complete
        {
            float* so = m.states + (((size_t)b * m.H + h) * m.nch + ch) * N * P;
            for (int k = tid; k < N * P; k += 256) so[k] = Ss[(k / P) * XS + k % P];
        }
        load_chunk<N>(m, b, h, c0, tid, Xs, Bs, Cs, dts);
        __syncthreads();
        if (wave == 0) chunk_decay(lane, A, dts, sv, es, fs, eL);
        __syncthreads();
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (jt <= it) {
                const float* ca = Cs + (32 * it + lrow) * BS + lhalf;
                const float* bb = Bs + (32 * jt + lrow) * BS + lhalf;
#pragma unroll 4
                for (int s = 0; s < NP / 2; ++s) acc = mfma32(ca[2 * s], bb[2 * s], acc);
            }
            const int j = 32 * jt + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * it + acc_row(r, lhalf);
                const bool keep = j <= i;
                const float e = expf(keep ? sv[i] - sv[j] : 0.f);
                Gs[i * XS + j] = keep ? acc[r] * e * dts[j] : 0.f;
            }
        }
        __syncthreads();
        {
            const int pt = jt, pc = 32 * pt + lrow;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* ca = Cs + (32 * it + lrow) * BS + lhalf;
#pragma unroll 4
            for (int s = 0; s < NP / 2; ++s) acc = mfma32(ca[2 * s], Ss[(2 * s + lhalf) * XS + pc], acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= es[32 * it + acc_row(r, lhalf)];
            const float* ga = Gs + (32 * it + lrow) * XS + lhalf;
            for (int s = 0; s < 16 * (it + 1); ++s) acc = mfma32(ga[2 * s], Xs[(2 * s + lhalf) * XS + pc], acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * it + acc_row(r, lhalf), t = c0 + i;
                if (t < L) m.ys[((size_t)b * L + t) * m.di + h * P + pc] = acc[r] + Dh * Xs[i * XS + pc];
            }
        }
        __syncthreads();                                                     // every read of S as an operand is done
        for (int tl = wave; tl < 2 * NT; tl += 4) {
            const int nt = tl >> 1, pc = 32 * (tl & 1) + lrow;
            const float e63 = eL[0];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = e63 * Ss[(32 * nt + acc_row(r, lhalf)) * XS + pc];
#pragma unroll 4
            for (int s = 0; s < Q / 2; ++s) {
                const int j = 2 * s + lhalf;
                acc = mfma32(Bs[j * BS + 32 * nt + lrow] * (fs[j] * dts[j]), Xs[j * XS + pc], acc);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) Ss[(32 * nt + acc_row(r, lhalf)) * XS + pc] = acc[r];
        }
    }
}

// out = norm.weight g rsqrt(mean_c g^2 + eps), g = ys silu(z); one wave per row, the sum of squares in wave_sum's fixed order
__global__ __launch_bounds__(256) void mtrain_gate_fwd_kernel(const float* __restrict__ ys, const float* __restrict__ zx, int ldz, int di,
                                                              const float* __restrict__ nw, float* __restrict__ out, size_t rows) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float ss = 0.f;
    for (int c = lane; c < di; c += 64) {
        const float g = ys[row * di + c] * silu(zx[row * ldz + c]);
        ss += g * g;
    }
    const float r = rsqrtf(wave_sum(ss) / (float)di + EPS);
    for (int c = lane; c < di; c += 64) out[row * di + c] = nw[c] * (ys[row * di + c] * silu(zx[row * ldz + c])) * r;
}

// ------------------------------------------------------------------------------------------------ backward
// Gate and norm of 64 rows per workgroup: with o = g r w, dg = r w do - g r^3 mean_c(g w do); dys = dg silu(z); dz = dg ys silu'(z);
// pnw[tile][c] = sum over the tile's rows of do g r (row order)
__global__ __launch_bounds__(256) void mtrain_gate_bwd_kernel(const float* __restrict__ ys, const float* __restrict__ zx, int ldz, int di,
                                                              const float* __restrict__ nw, const float* __restrict__ dout,
                                                              float* __restrict__ dys, float* __restrict__ dzx, float* __restrict__ pnw,
                                                              size_t rows) {
    __shared__ float rr[64], mm[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * 64;
    for (int i = wave; i < 64; i += 4) {
        const size_t row = r0 + i;
        float ss = 0.f, sg = 0.f;
        if (row < rows)
            for (int c = lane; c < di; c += 64) {
                const float g = ys[row * di + c] * silu(zx[row * ldz + c]);
                ss += g * g;
                sg += g * nw[c] * dout[row * di + c];
            }
        ss = wave_sum(ss), sg = wave_sum(sg);
        const float r = rsqrtf(ss / (float)di + EPS);
        if (lane == 0) rr[i] = r, mm[i] = r * r * r * (sg / (float)di);
    }
    __syncthreads();
    for (int c = 4 * tid; c < di; c += 1024) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(nw + c);
        f32x4 dw = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 64 && r0 + i < rows; ++i) {
            const size_t row = r0 + i;
            const f32x4 y4 = *reinterpret_cast<const f32x4*>(ys + row * di + c), z4 = *reinterpret_cast<const f32x4*>(zx + row * ldz + c);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(dout + row * di + c);
            const float r = rr[i], mg = mm[i];
            f32x4 dy4, dz4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sz = silu(z4[e]), g = y4[e] * sz, dg = r * w4[e] * d4[e] - g * mg;
                dy4[e] = dg * sz;
                dz4[e] = dg * y4[e] * dsilu(z4[e]);
                dw[e] += d4[e] * g * r;
            }
            *reinterpret_cast<f32x4*>(dys + row * di + c) = dy4;
            *reinterpret_cast<f32x4*>(dzx + row * ldz + c) = dz4;
        }
        *reinterpret_cast<f32x4*>(pnw + (size_t)blockIdx.x * di + c) = dw;
    }
}

// One workgroup (4 waves) per (read, head), walking the chunks in reverse.  dS is the gradient of the chunk's exit state (zero after
// the last chunk), S_in its entry state as the forward left it.  With Lm_ij = exp(s_i - s_j) (j <= i, else exactly 0), e = exp(s),
// f_j = exp(s_63 - s_j), CB = C B^T, DX = dys X^T, G = Lm dt_j CB, W = Lm dt_j DX, Kl = Lm CB DX:
//   dx  = G^T dys + f dt (B dS) + D dys        dC = e (dys S_in^T) + W B        dB = f dt (X dS^T) + W^T C
//   r_i = C_i . (e_i dys_i S_in^T)   ub_j = f_j B_j . (X dS^T)_j   u = dt ub
//   ds_i = sum_j K_ij - sum_k K_ki + r_i - u_i ;  ds_63 += sum_j u_j + e_63 <dS, S_in> ;  da = reverse cumulative sum of ds
//   ddt_j = sum_i Kl_ij + ub_j + A da_j ;  dA += sum da dt ;  dD += sum dys . x ;  dS <- e_63 dS + (e C)^T dys
template <int N>
__global__ __launch_bounds__(256) void mtrain_scan_bwd_kernel(ScanArgs m) {
    using SH = ScanShape<N>;
    constexpr int NP = SH::NP, NT = SH::NT, BS = SH::BS;
    extern __shared__ __attribute__((aligned(16))) float smem_mt[];
    float* Xs = smem_mt;                 // [Q][XS] x
    float* Ys = Xs + Q * XS;             // [Q][XS] dys
    float* Gs = Ys + Q * XS;             // [Q][XS] G, then W
    float* Bs = Gs + Q * XS;             // [Q][BS]
    float* Cs = Bs + Q * BS;             // [Q][BS]
    float* dSs = Cs + Q * BS;            // [NP][XS] dS, n-major
    float* sv = dSs + NP * XS;
    float* es = sv + Q;
    float* fs = es + Q;
    float* dts = fs + Q;
    float* rsK = dts + Q;                // [2][Q] row sums of K over each column tile
    float* csKl = rsK + 2 * Q;           // [2][Q] column sums of Kl over each row tile
    float* csK = csKl + 2 * Q;           // [2][Q] column sums of K (the products the row sums add: a lone token's ds is exactly 0)
    float* rP = csK + 2 * Q;             // [4][Q] r_i per 32-column tile of N
    float* uP = rP + 4 * Q;              // [4][Q] ub_j likewise
    float* red = uP + 4 * Q;             // [2][256] per-thread partials of <dS, S_in> and of dys . x
    float* eL = red + 512;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lrow = lane & 31, lhalf = lane >> 5;
    const int h = (int)blockIdx.x % m.H, b = (int)blockIdx.x / m.H, L = m.L;
    const float A = -expf(m.A_log[h]), Dh = m.Dp[h];
    for (int k = tid; k < 2 * Q * BS + NP * XS; k += 256) Bs[k] = 0.f;      // padding columns; dS = 0 behind the last chunk
    for (int k = tid; k < 8 * Q; k += 256) rP[k] = 0.f;                      // tiles of N that do not exist contribute 0
    const int it = wave >> 1, jt = wave & 1;
    float dA_acc = 0.f, dD_acc = 0.f;                                        // (wave 0)
    for (int ch = m.nch - 1; ch >= 0; --ch) {
        const int c0 = ch * Q;
        const float* Sin = m.states + (((size_t)b * m.H + h) * m.nch + ch) * N * P;
        __syncthreads();                                                     // the chunk behind is finished with everything in LDS
        load_chunk<N>(m, b, h, c0, tid, Xs, Bs, Cs, dts);
        for (int k = tid; k < Q * P; k += 256) {
            const int i = k / P, p = k % P, t = c0 + i;
            Ys[i * XS + p] = t < L ? m.dys[((size_t)b * L + t) * m.di + h * P + p] : 0.f;
        }
        __syncthreads();
        if (wave == 0) chunk_decay(lane, A, dts, sv, es, fs, eL);
        __syncthreads();
        // ---- this wave's tile (rows i of tile it, columns j of tile jt) of CB and DX -> G (to LDS), W (kept), sums of K and Kl
        f32x16 Wt;
        {
            f32x16 cb, dx;
#pragma unroll
            for (int r = 0; r < 16; ++r) cb[r] = 0.f, dx[r] = 0.f;
            if (jt <= it) {
                const float* ca = Cs + (32 * it + lrow) * BS + lhalf;
                const float* bb = Bs + (32 * jt + lrow) * BS + lhalf;
#pragma unroll 4
                for (int s = 0; s < NP / 2; ++s) cb = mfma32(ca[2 * s], bb[2 * s], cb);
                const float* ya = Ys + (32 * it + lrow) * XS + lhalf;
                const float* xb = Xs + (32 * jt + lrow) * XS + lhalf;
#pragma unroll 4
                for (int s = 0; s < P / 2; ++s) dx = mfma32(ya[2 * s], xb[2 * s], dx);
            }
            const int j = 32 * jt + lrow;
            const float dtj = dts[j], sj = sv[j];
            float col = 0.f, colk = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * it + acc_row(r, lhalf);
                const bool keep = j <= i;
                const float lm = keep ? expf(sv[i] - sj) : 0.f;             // (the difference is <= 0 wherever it is used)
                const float kl = keep ? lm * cb[r] * dx[r] : 0.f;
                Gs[i * XS + j] = keep ? lm * dtj * cb[r] : 0.f;
                Wt[r] = keep ? lm * dtj * dx[r] : 0.f;
                const float kk = kl * dtj;
                col += kl;
                colk += kk;
                const float rs = half_sum(kk);
                if (lrow == 0) rsK[jt * Q + i] = rs;
            }
            col += __shfl_xor(col, 32, 64);
            colk += __shfl_xor(colk, 32, 64);
            if (lhalf == 0) csKl[it * Q + j] = col, csK[it * Q + j] = colk;
        }
        __syncthreads();
        // ---- dx tile (rows j of tile it, channels of tile jt)
        {
            const int pc = 32 * jt + lrow;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* ba = Bs + (32 * it + lrow) * BS + lhalf;
#pragma unroll 4
            for (int s = 0; s < NP / 2; ++s) acc = mfma32(ba[2 * s], dSs[(2 * s + lhalf) * XS + pc], acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * it + acc_row(r, lhalf);
                acc[r] *= fs[j] * dts[j];
            }
            for (int s = 16 * it; s < Q / 2; ++s) {                          // (G_ij = 0 for i < j: rows before this tile's add nothing)
                const int i = 2 * s + lhalf;
                acc = mfma32(Gs[i * XS + 32 * it + lrow], Ys[i * XS + pc], acc);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * it + acc_row(r, lhalf), t = c0 + j;
                if (t < L) m.dx[((size_t)b * L + t) * m.di + h * P + pc] = acc[r] + Dh * Ys[j * XS + pc];
            }
        }
        __syncthreads();                                                     // G has been read: W takes its place
        {
            const int j = 32 * jt + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) Gs[(32 * it + acc_row(r, lhalf)) * XS + j] = Wt[r];
        }
        __syncthreads();
        // ---- dC and dB tiles: 2 row tiles x NT column tiles each, dealt to the waves in a fixed order
        for (int tl = wave; tl < 4 * NT; tl += 4) {
            const int kind = tl / (2 * NT), rt = (tl % (2 * NT)) / NT, nt = tl % NT, nc = 32 * nt + lrow;
            float* dst = m.dbc + (((size_t)b * m.H + h) * L) * 2 * N + (kind == 0 ? N : 0) + nc;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (kind == 0) {
                // dC: e_i (dys_i S_in^T): the contraction runs over p = 32 lhalf + s, so a lane reads 32 consecutive floats of its state row
                const float* ya = Ys + (32 * rt + lrow) * XS + 32 * lhalf;
                const float* sb = Sin + (size_t)(nc < N ? nc : 0) * P + 32 * lhalf;
                const float live = nc < N ? 1.f : 0.f;
#pragma unroll
                for (int s4 = 0; s4 < 8; ++s4) {
                    const f32x4 sq = *reinterpret_cast<const f32x4*>(sb + 4 * s4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = mfma32(ya[4 * s4 + e], sq[e] * live, acc);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = 32 * rt + acc_row(r, lhalf);
                    acc[r] *= es[i];
                    const float rs = half_sum(acc[r] * Cs[i * BS + nc]);
                    if (lrow == 0) rP[nt * Q + i] = rs;
                }
                const float* wa = Gs + (32 * rt + lrow) * XS + lhalf;
                for (int s = 0; s < 16 * (rt + 1); ++s) acc = mfma32(wa[2 * s], Bs[(2 * s + lhalf) * BS + nc], acc);
            } else {
                const float* xa = Xs + (32 * rt + lrow) * XS + lhalf;
                const float* db = dSs + nc * XS + lhalf;
#pragma unroll 4
                for (int s = 0; s < P / 2; ++s) acc = mfma32(xa[2 * s], db[2 * s], acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * rt + acc_row(r, lhalf);
                    const float us = half_sum(fs[j] * acc[r] * Bs[j * BS + nc]);
                    if (lrow == 0) uP[nt * Q + j] = us;
                    acc[r] *= fs[j] * dts[j];
                }
                for (int s = 16 * rt; s < Q / 2; ++s) {
                    const int i = 2 * s + lhalf;
                    acc = mfma32(Gs[i * XS + 32 * rt + lrow], Cs[i * BS + nc], acc);
                }
            }
            if (nc < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int t = c0 + 32 * rt + acc_row(r, lhalf);
                    if (t < L) dst[(size_t)t * 2 * N] = acc[r];
                }
            }
        }
        // per-thread partials of dys . x (a quarter row each)
        {
            const int i = tid >> 2, p0 = 16 * (tid & 3);
            float s = 0.f;
#pragma unroll
            for (int p = 0; p < 16; ++p) s += Ys[i * XS + p0 + p] * Xs[i * XS + p0 + p];
            red[256 + tid] = s;
        }
        __syncthreads();                                                     // every read of dS as an operand is done
        // ---- <dS, S_in> and dS <- e_63 dS + (e C)^T dys, a tile at a time in place
        {
            float dot = 0.f;
            for (int tl = wave; tl < 2 * NT; tl += 4) {
                const int nt = tl >> 1, pc = 32 * (tl & 1) + lrow;
                const float e63 = eL[0];
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = 32 * nt + acc_row(r, lhalf);
                    const float d = dSs[n * XS + pc];
                    if (n < N) dot += d * Sin[(size_t)n * P + pc];
                    acc[r] = e63 * d;
                }
#pragma unroll 4
                for (int s = 0; s < Q / 2; ++s) {
                    const int i = 2 * s + lhalf;
                    acc = mfma32(Cs[i * BS + 32 * nt + lrow] * es[i], Ys[i * XS + pc], acc);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dSs[(32 * nt + acc_row(r, lhalf)) * XS + pc] = acc[r];
            }
            red[tid] = dot;
        }
        __syncthreads();
        // ---- the decay's gradient: lane i of wave 0 owns token i of the chunk
        if (wave == 0) {
            const int i = lane, t = c0 + i;
            const float dti = dts[i];
            const float ckl = csKl[i] + csKl[Q + i];
            const float ri = (rP[i] + rP[Q + i]) + (rP[2 * Q + i] + rP[3 * Q + i]);
            const float ub = (uP[i] + uP[Q + i]) + (uP[2 * Q + i] + uP[3 * Q + i]);
            const float u = ub * dti;
            float ds = (rsK[i] + rsK[Q + i]) - (csK[i] + csK[Q + i]) + ri - u;
            const float usum = wave_sum(u);
            const float dot = wave_sum((red[4 * i] + red[4 * i + 1]) + (red[4 * i + 2] + red[4 * i + 3]));
            const float dyx = wave_sum((red[256 + 4 * i] + red[257 + 4 * i]) + (red[258 + 4 * i] + red[259 + 4 * i]));
            if (i == Q - 1) ds += usum + eL[0] * dot;
            float da = ds;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float v = __shfl_down(da, o, 64);
                if (lane + o < 64) da += v;
            }
            if (t < L) m.ddt[((size_t)b * L + t) * m.H + h] = ckl + ub + A * da;
            dA_acc += wave_sum(da * dti);
            dD_acc += dyx;
        }
    }
    if (tid == 0) {
        m.pA[(size_t)b * m.H + h] = A * dA_acc;                              // dA_log = A dA
        m.pD[(size_t)b * m.H + h] = dD_acc;
    }
}

// SiLU and the four taps backwards inside the read; one thread per channel walks a 64-token tile (and the three rows behind it, whose
// du its last rows need).  dxc of a B / C column is the sum of the heads' parts in head order.  du_t = dxc_t silu'(u_t);
// dxBC_t = sum_k w_k du_{t + 3 - k};  pcw[tile][c][k] = sum_t du_t xBC_{t - 3 + k},  pcb[tile][c] = sum_t du_t  (the tile's own rows)
__global__ __launch_bounds__(256) void mtrain_conv_bwd_kernel(const float* __restrict__ zx, int ldz, int di, int conv_dim, int N, int H,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ dx, const float* __restrict__ dbc,
                                                              float* __restrict__ dzx, float* __restrict__ pcw, float* __restrict__ pcb,
                                                              int L, int tiles_x, int cblocks) {
    const int cb = (int)blockIdx.x % cblocks, tile = (int)blockIdx.x / cblocks;
    const int c = cb * 256 + (int)threadIdx.x;
    if (c >= conv_dim) return;
    const int b = tile / tiles_x, t0 = (tile % tiles_x) * 64;
    const size_t rb = (size_t)b * L;
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + 4 * c);
    const float bc = bias[c];
    auto xin = [&](int t) { return t >= 0 && t < L ? zx[(rb + t) * ldz + di + c] : 0.f; };
    auto dxc = [&](int t) {
        if (c < di) return dx[(rb + t) * di + c];
        float s = 0.f;
        for (int hh = 0; hh < H; ++hh) s += dbc[(((size_t)b * H + hh) * L + t) * 2 * N + (c - di)];
        return s;
    };
    float xm3 = xin(t0 - 3), xm2 = xin(t0 - 2), xm1 = xin(t0 - 1);
    float d3 = 0.f, d2 = 0.f, d1 = 0.f;                                      // du of t - 3, t - 2, t - 1
    f32x4 aw = {0.f, 0.f, 0.f, 0.f};
    float ab = 0.f;
    const int tend = t0 + 64 < L ? t0 + 64 : L;
    for (int t = t0; t < tend + 3; ++t) {
        const float xt = xin(t);
        float d0 = 0.f;
        if (t < L) {
            float u = bc;
            u += w4[0] * xm3, u += w4[1] * xm2, u += w4[2] * xm1, u += w4[3] * xt;
            d0 = dxc(t) * dsilu(u);
            if (t < tend) aw[0] += d0 * xm3, aw[1] += d0 * xm2, aw[2] += d0 * xm1, aw[3] += d0 * xt, ab += d0;
        }
        if (t - 3 >= t0) dzx[(rb + t - 3) * ldz + di + c] = w4[3] * d3 + w4[2] * d2 + w4[1] * d1 + w4[0] * d0;
        d3 = d2, d2 = d1, d1 = d0;
        xm3 = xm2, xm2 = xm1, xm1 = xt;
    }
    *reinterpret_cast<f32x4*>(pcw + ((size_t)tile * conv_dim + c) * 4) = aw;
    pcb[(size_t)tile * conv_dim + c] = ab;
}

// d raw = ddt sigmoid(raw + dt_bias) over 64 rows per workgroup; pdt[tile][h] = their sum in row order
__global__ __launch_bounds__(64) void mtrain_dt_bwd_kernel(const float* __restrict__ zx, int ldz, int dt0, int H,
                                                           const float* __restrict__ dt_bias, const float* __restrict__ ddt,
                                                           float* __restrict__ dzx, float* __restrict__ pdt, size_t rows) {
    const size_t r0 = (size_t)blockIdx.x * 64;
    for (int hh = threadIdx.x; hh < H; hh += 64) {
        const float bh = dt_bias[hh];
        float s = 0.f;
        for (int i = 0; i < 64 && r0 + i < rows; ++i) {
            const size_t row = r0 + i;
            const float g = ddt[row * H + hh] * sigm(zx[row * ldz + dt0 + hh] + bh);
            dzx[row * ldz + dt0 + hh] = g;
            s += g;
        }
        pdt[(size_t)blockIdx.x * H + hh] = s;
    }
}

// out[c] = the sum of part[i][c] over the workgroups' partials i = 0 .. nparts - 1, in that order, in fp64
__global__ __launch_bounds__(256) void mtrain_reduce_kernel(const float* __restrict__ part, int nparts, size_t width, float* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= width) return;
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += (double)part[(size_t)i * width + c];
    out[c] = (float)s;
}

template <bool BWD>
void launch_scan(const ScanArgs& m, int N, int reads, hipStream_t st) {
    const dim3 grid((unsigned)((size_t)m.H * reads)), block(256);
#define CLM_MT_CASE(NN)                                                                                             \
    case NN:                                                                                                        \
        if constexpr (BWD) launch_lds<mtrain_scan_bwd_kernel<NN>>(grid, block, bwd_lds<NN>, st, m);          \
        else launch_lds<mtrain_scan_fwd_kernel<NN>>(grid, block, fwd_lds<NN>, st, m);                        \
        break;
    switch (N) {
        CLM_MT_CASE(16)
        CLM_MT_CASE(32)
        CLM_MT_CASE(64)
        default:
            CLM_MT_CASE(128)
    }
#undef CLM_MT_CASE
}

}  // namespace mtrain
}  // namespace clm

// ================================================================================================ C ABI
using namespace clm;

struct clm_mamba_train_handle {
    int device = 0;
    std::string err;
    DevBuf ws;                      // the backward's scratch (clm_mamba_train_workspace_bytes), grown on demand
};

namespace {

struct Dims {
    int B, L, d, N, di, H, conv_dim, ldz, nch, tiles_x;
    size_t rows, tiles;
};

// CLM_OK and the derived sizes, or the refusal (nothing has been launched)
int train_dims(clm_mamba_train_handle* h, const char* who, int B, int L, int d_model, int expand, int d_state, Dims& q) {
    const std::string w(who);
    if (B < 1 || L < 1) return fail(h, CLM_E_INVALID, w + ": B and L must be at least 1");
    const bool ok = (d_model == 256 || d_model == 512) && (d_state == 16 || d_state == 32 || d_state == 64 || d_state == 128) && expand >= 1 &&
                    expand <= 1024;
    if (!ok)
        return fail(h, CLM_E_UNSUPPORTED, w + ": supported shapes are d_model 256 or 512, d_state 16 / 32 / 64 / 128, headdim 64 and an "
                                              "integer expand in 1 ... 1024");
    q.B = B, q.L = L, q.d = d_model, q.N = d_state, q.di = expand * d_model, q.H = q.di / ssm::P;
    q.conv_dim = q.di + 2 * d_state, q.ldz = 2 * q.di + 2 * d_state + q.H;
    q.nch = q.tiles_x = (L + 63) / 64;
    q.rows = (size_t)B * L;
    q.tiles = (size_t)B * q.tiles_x;
    // every launch grid must fit 2^31 - 1 workgroups (element offsets are 64 bits wide throughout)
    const size_t lim = 0x7fffffffull;
    const size_t worst = std::max({q.rows * ((size_t)q.conv_dim / 4 + q.H) / 256 + 1, q.tiles * (((size_t)q.conv_dim + 255) / 256), (size_t)B * q.H});
    if (q.rows > lim || worst > lim) return fail(h, CLM_E_UNSUPPORTED, w + ": the batch is beyond the kernels' index range (B L < 2^31 and every grid < 2^31)");
    return CLM_OK;
}

size_t ws_floats(const Dims& q) {
    return q.rows * ((size_t)2 * q.di + q.H) + q.rows * (size_t)q.H * 2 * q.N + q.tiles * ((size_t)q.di + 5 * (size_t)q.conv_dim + q.H) +
           (size_t)2 * q.B * q.H;
}

}  // namespace

extern "C" {

int clm_mamba_train_create(int device, clm_mamba_train_handle** out) {
    if (!out) return fail<clm_mamba_train_handle>(nullptr, CLM_E_INVALID, "clm_mamba_train_create: bad argument");
    if (int rc = use_gfx950<clm_mamba_train_handle>(device, "clm_mamba_train_create")) return rc;
    clm_mamba_train_handle* h = new clm_mamba_train_handle();
    h->device = device;
    *out = h;
    return CLM_OK;
}

int64_t clm_mamba_train_workspace_bytes(int B, int L, int d_model, int expand, int d_state) {
    clm_mamba_train_handle tmp;
    Dims q;
    if (int rc = train_dims(&tmp, "clm_mamba_train_workspace_bytes", B, L, d_model, expand, d_state, q)) return rc;
    return (int64_t)(ws_floats(q) * 4);
}

int clm_mamba_train_forward(clm_mamba_train_handle* h, const float* zxbcdt, const float* const* params, int B, int L, int d_model,
                            int expand, int d_state, float* xc, float* dt, float* ys, float* states, float* out, void* stream) {
    if (!h) return CLM_E_INVALID;
    Dims q;
    if (int rc = train_dims(h, "clm_mamba_train_forward", B, L, d_model, expand, d_state, q)) return rc;
    if (!zxbcdt || !params || !xc || !dt || !ys || !states || !out) return fail(h, CLM_E_INVALID, "clm_mamba_train_forward: null argument");
    for (int i = 0; i < CLM_MAMBA_TRAIN_PARAMS; ++i)
        if (!params[i]) return fail(h, CLM_E_INVALID, "clm_mamba_train_forward: null parameter");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *cw = params[0], *cbias = params[1], *dtb = params[2], *alog = params[3], *Dp = params[4], *nw = params[5];
    const size_t items = q.rows * ((size_t)q.conv_dim / 4 + q.H);
    hipLaunchKernelGGL(mtrain::mtrain_pre_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, zxbcdt, q.ldz, q.di, q.conv_dim,
                       q.H, cw, cbias, dtb, xc, dt, q.rows, L);
    mtrain::ScanArgs s{};
    s.xc = xc, s.ldx = q.conv_dim, s.dt = dt, s.A_log = alog, s.Dp = Dp, s.ys = ys, s.states = states, s.L = L, s.di = q.di, s.H = q.H, s.nch = q.nch;
    mtrain::launch_scan<false>(s, q.N, B, st);
    hipLaunchKernelGGL(mtrain::mtrain_gate_fwd_kernel, dim3((unsigned)((q.rows + 3) / 4)), dim3(256), 0, st, ys, zxbcdt, q.ldz, q.di, nw, out,
                       q.rows);
    return launched(h, "clm_mamba_train_forward");
}

int clm_mamba_train_backward(clm_mamba_train_handle* h, const float* zxbcdt, const float* const* params, int B, int L, int d_model,
                             int expand, int d_state, const float* xc, const float* dt, const float* ys, const float* states,
                             const float* dout, float* dzxbcdt, float* const* dparams, void* stream) {
    if (!h) return CLM_E_INVALID;
    Dims q;
    if (int rc = train_dims(h, "clm_mamba_train_backward", B, L, d_model, expand, d_state, q)) return rc;
    if (!zxbcdt || !params || !xc || !dt || !ys || !states || !dout || !dzxbcdt || !dparams)
        return fail(h, CLM_E_INVALID, "clm_mamba_train_backward: null argument");
    for (int i = 0; i < CLM_MAMBA_TRAIN_PARAMS; ++i)
        if (!params[i] || !dparams[i]) return fail(h, CLM_E_INVALID, "clm_mamba_train_backward: null parameter or gradient");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = grow(h, Sync::Device(), {{&h->ws, ws_floats(q) * 4}})) return rc;   // (queued kernels of an earlier call may still read the old scratch)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float *cw = params[0], *cbias = params[1], *dtb = params[2], *alog = params[3], *Dp = params[4], *nw = params[5];
    float* p = h->ws.get<float>();
    float* dys = p; p += q.rows * q.di;
    float* dx = p; p += q.rows * q.di;
    float* ddt = p; p += q.rows * q.H;
    float* dbc = p; p += q.rows * (size_t)q.H * 2 * q.N;
    float* pnw = p; p += q.tiles * q.di;
    float* pcw = p; p += q.tiles * (size_t)q.conv_dim * 4;
    float* pcb = p; p += q.tiles * (size_t)q.conv_dim;
    float* pdt = p; p += q.tiles * q.H;
    float* pA = p; p += (size_t)B * q.H;
    float* pD = p;
    const unsigned t64 = (unsigned)((q.rows + 63) / 64);        // 64-row tiles of the flat row index (<= q.tiles)
    hipLaunchKernelGGL(mtrain::mtrain_gate_bwd_kernel, dim3(t64), dim3(256), 0, st, ys, zxbcdt, q.ldz, q.di, nw, dout, dys, dzxbcdt, pnw, q.rows);
    mtrain::ScanArgs s{};
    s.xc = xc, s.ldx = q.conv_dim, s.dt = dt, s.A_log = alog, s.Dp = Dp, s.states = const_cast<float*>(states), s.dys = dys, s.dx = dx;
    s.ddt = ddt, s.dbc = dbc, s.pA = pA, s.pD = pD, s.L = L, s.di = q.di, s.H = q.H, s.nch = q.nch;
    mtrain::launch_scan<true>(s, q.N, B, st);
    const int cblocks = (q.conv_dim + 255) / 256;
    hipLaunchKernelGGL(mtrain::mtrain_conv_bwd_kernel, dim3((unsigned)(q.tiles * cblocks)), dim3(256), 0, st, zxbcdt, q.ldz, q.di, q.conv_dim,
                       q.N, q.H, cw, cbias, dx, dbc, dzxbcdt, pcw, pcb, L, q.tiles_x, cblocks);
    hipLaunchKernelGGL(mtrain::mtrain_dt_bwd_kernel, dim3(t64), dim3(64), 0, st, zxbcdt, q.ldz, q.di + q.conv_dim, q.H, dtb, ddt, dzxbcdt, pdt,
                       q.rows);
    auto reduce = [&](const float* part, size_t nparts, size_t width, float* out) {
        hipLaunchKernelGGL(mtrain::mtrain_reduce_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, st, part, (int)nparts, width, out);
    };
    reduce(pcw, q.tiles, (size_t)q.conv_dim * 4, dparams[0]);
    reduce(pcb, q.tiles, (size_t)q.conv_dim, dparams[1]);
    reduce(pdt, t64, (size_t)q.H, dparams[2]);
    reduce(pA, (size_t)B, (size_t)q.H, dparams[3]);
    reduce(pD, (size_t)B, (size_t)q.H, dparams[4]);
    reduce(pnw, t64, (size_t)q.di, dparams[5]);
    return launched(h, "clm_mamba_train_backward");
}

const char* clm_mamba_train_last_error(const clm_mamba_train_handle* h) {
    return h ? h->err.c_str() : create_error<clm_mamba_train_handle>().c_str();
}

int clm_mamba_train_destroy(clm_mamba_train_handle* h) { return destroy_handle(h); }

}  // extern "C"
