// attention_train.hip -- the attention core of SequenceCNNTransformer for training: the exact-fp32 tiled
// forward of attention.hip with the log-sum-exp as a second output and dropout on the probabilities, and its backward.  Stateless:
// the caller owns every tensor (chimeralm_amd/tftrain.py holds them in the autograd node).
//
//   forward    s_ij = q_i . k_j / sqrt(32),  p_ij = 2^(s_ij log2 e - lse_i),  lse_i = log2 sum_j exp(s_ij)      (LOG2 units: what
//              the kernels' exp2 takes as it is -- no second rounding of the exponent on the way back into the backward)
//              O_i  = sum_j keep_ij p_ij v_j / (1 - p_drop)
//   backward   delta_i = sum_d dO_id O_id                                  (= sum_j p_ij dS'_ij: holds with dropout)
//              dP_ij = dO_i . v_j,   dS_ij = p_ij (keep_ij dP_ij / (1 - p_drop) - delta_i)
//              dQ_i = sum_j dS_ij k_j / sqrt(32),  dK_j = sum_i dS_ij q_i / sqrt(32),  dV_j = sum_i keep_ij p_ij dO_i / (1 - p_drop)
//
// The forward IS attention_tiles<A32> (attention_tiles.h) with the keep mask as its per-tile hook; without dropout it is
// attention32_kernel's arithmetic to the bit.  The backward never runs an online softmax: lse is known, P is recomputed as
// exp2(s c - lse).  It is two passes, each shaped like the forward -- the index a lane owns stays in the lanes, the streamed
// index sits in the accumulator rows, so the accumulator registers are the B operand of the next product:
//   dq pass       per 128-query tile over 64-key tiles:   S^T = K Q^T, dP^T = V dO^T (A operand: rows of the staged tile), dS^T in
//                 place, dQ^T += K^T dS^T (A operand: columns of the same staged K tile)
//   dk | dv pass  per 128-key tile over 64-query tiles:   S = Q K^T, dP = dO V^T, dV^T += dO^T P', dK^T += Q^T dS
// 112 MFMAs of v_mfma_f32_32x32x2_f32 per 32 x 32 block against the forward's 32: S and dP are computed in both passes so that no
// pass adds into another's output -- no floating-point atomics, two calls give the same bits.
//
// The keep mask is a pure function of (seed, b * 8 + h, i, j), mask_row() / mask_keep() below (restated in tests/attention_train_reference.py):
// the backward regenerates it, nothing quadratic is ever stored outside clm_attn_train_mask.
#include "attention_tiles.h"

namespace clm {

namespace {

constexpr float INV_SQRT_HD = 0.17677669529663687f;   // 1 / sqrt(32)
constexpr float LOG2E = 1.4426950408889634f;
constexpr int TRS = KRS32;        // row stride of the backward's staged tiles: ds_read_b128 of 16 rows on 16 bank groups

// ---- the keep mask.  mix32 is a 32-bit avalanche mixer (xor-shift / odd-multiply, "lowbias32"); bits() applies it twice:
//   r    = mix32(seed_lo ^ i * 0x9E3779B1)
//   bits = mix32((r ^ (seed_hi + bh * 0x85EBCA77)) + j * 0xC2B2AE3D)                (all arithmetic modulo 2^32)
//   keep = bits >= round(p * 2^32)
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
struct MaskKey {
    uint32_t lo, hi, thr;
};
__device__ __forceinline__ uint32_t mask_row(const MaskKey& k, int bh, int i) {   // everything of bits() that does not depend on j
    return mix32(k.lo ^ ((uint32_t)i * 0x9E3779B1u)) ^ (k.hi + (uint32_t)bh * 0x85EBCA77u);
}
__device__ __forceinline__ bool mask_keep(const MaskKey& k, uint32_t row, int j) {
    return mix32(row + (uint32_t)j * 0xC2B2AE3Du) >= k.thr;
}

// the forward's hook: zero the dropped probabilities of this lane's query (keys beyond L are 0 already)
struct DropHook {
    MaskKey key;
    __device__ __forceinline__ void tile(f32x16 (&p)[2], int bh, int q, int k0, int hf) const {
        const uint32_t row = mask_row(key, bh, q);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (!mask_keep(key, row, k0 + blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf)) p[blk][r] = 0.f;
    }
};

template <bool DROP>
__global__ __launch_bounds__(256, 4) void attn_train_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                float* __restrict__ lse, int L, MaskKey key, float rscale) {
    __shared__ __attribute__((aligned(16))) float Ks[2][KT * KRS32];
    __shared__ __attribute__((aligned(16))) float Vs[2][KT * VRS32];
    A32 a;
    a.Ks = &Ks[0][0], a.Vs = &Vs[0][0];
    f32x16 o;
    float inv, m, lsum;
    int b, h, q;
    if constexpr (DROP) {
        attention_tiles(a, DropHook{key}, qkv, L, o, inv, m, lsum, b, h, q);
        inv *= rscale;
    } else {
        attention_tiles(a, NoHook{}, qkv, L, o, inv, m, lsum, b, h, q);
    }
    store_f32(out, L, o, inv, b, h, q);
    // lse = m c + log2 l, rounded ONCE (the sum in fp64): the backward's p = exp2(s c - lse) inherits lse's absolute error as its own
    // relative error, and half an ulp of a value of ~6 is already 1.4 ... 2.8 ulp of p.  m c is the product as the loop rounded it.
    if (q < L && !(threadIdx.x & 32)) {
        const float mc = m * (LOG2E * INV_SQRT_HD);
        lse[((size_t)b * NH + h) * L + q] = (float)((double)mc + log2((double)lsum));
    }
}

// delta[b, h, i] = sum_d dO[b, i, h * 32 + d] O[b, i, h * 32 + d], summed in d order: one thread per (row, head)
__global__ __launch_bounds__(256) void attn_train_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                               float* __restrict__ delta, int B, int L) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * L * NH) return;
    const int h = (int)(idx & 7);
    const size_t row = idx >> 3;
    const float4* o = reinterpret_cast<const float4*>(out + row * D + h * HD);
    const float4* g = reinterpret_cast<const float4*>(dout + row * D + h * HD);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
        const float4 x = o[i], y = g[i];
        s = fmaf(x.x, y.x, s), s = fmaf(x.y, y.y, s), s = fmaf(x.z, y.z, s), s = fmaf(x.w, y.w, s);
    }
    const size_t b = row / L, i = row % L;
    delta[(b * NH + h) * L + i] = s;
}

// ---- the backward's staging: 64 rows x 32 floats of two row-major arrays (strides xs, ys floats) into registers, then into LDS
struct Stage2 {
    f32x4 xr[2], yr[2];
    __device__ __forceinline__ void load(const float* xb, int xs, const float* yb, int ys, int r0, int L, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * 256, j = e >> 3, d4 = e & 7;
            const size_t row = r0 + j < L ? r0 + j : L - 1;             // clamped; the clones' probabilities are set to 0
            xr[i] = *reinterpret_cast<const f32x4*>(xb + row * xs + 4 * d4);
            yr[i] = *reinterpret_cast<const f32x4*>(yb + row * ys + 4 * d4);
        }
    }
    __device__ __forceinline__ void store(float* X, float* Y, int tid) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * 256, j = e >> 3, d4 = e & 7;
            *reinterpret_cast<f32x4*>(&X[j * TRS + 4 * d4]) = xr[i];
            *reinterpret_cast<f32x4*>(&Y[j * TRS + 4 * d4]) = yr[i];
        }
    }
};
// a lane's own row as B operand of the 16 k-steps: f[s][j] is d = 8 s + 4 hf + j
__device__ __forceinline__ void load_frag(f32x4 (&f)[4], const float* row, int hf) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const f32x4*>(row + 4 * hf + 8 * s);
}
// C[r][lane] = sum_d T[blk * 32 + r][d] f[d]: the rows of the staged tile T against the lane's own row (A32::scores)
__device__ __forceinline__ f32x16 rows_dot(const float* T, int blk, int n, int hf, const f32x4 (&f)[4]) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const float* tp = T + (blk * 32 + n) * TRS + 4 * hf;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const f32x4 tf = *reinterpret_cast<const f32x4*>(tp + 8 * st);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[j], f[st][j], s, 0, 0, 0);
    }
    return s;
}
// o[d][lane] += sum_r T[blk * 32 + r][d] p[r][lane]: p in accumulator layout is the B operand as it is (A32::pv)
__device__ __forceinline__ void cols_acc(const float* T, int blk, int n, int hf, const f32x16& p, f32x16& o) {
    const float* tp = T + (blk * 32 + 4 * hf) * TRS + n;
#pragma unroll
    for (int t = 0; t < 16; ++t) o = __builtin_amdgcn_mfma_f32_32x32x2f32(tp[((t & 3) + 8 * (t >> 2)) * TRS], p[t], o, 0, 0, 0);
}
// a lane's accumulator column (d = (r & 3) + 8 (r >> 2) + 4 hf) times sc to a 32-float row of dqkv
__device__ __forceinline__ void store_grad(float* row, const f32x16& o, float sc, int hf) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(row + 4 * hf + 8 * g) = make_float4(o[4 * g + 0] * sc, o[4 * g + 1] * sc, o[4 * g + 2] * sc, o[4 * g + 3] * sc);
}
// workgroup -> (tile of 128 owned rows, head, read): attention_tiles' XCD-aware order
__device__ __forceinline__ void tile_of(int L, int& bh, int& r0) {
    const int ntq = (L + QT - 1) / QT;
    const int g = blockIdx.x, xcd = g & 7, slot = g >> 3;
    bh = (slot / ntq) * 8 + xcd;
    r0 = (slot % ntq) * QT;
}

// ---- dq pass: a lane owns one query, the keys are streamed
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_train_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                               const float* __restrict__ delta, const float* __restrict__ dout,
                                                               float* __restrict__ dqkv, int L, MaskKey key, float rscale) {
    __shared__ __attribute__((aligned(16))) float Ks[2][KT * TRS];
    __shared__ __attribute__((aligned(16))) float Vs[2][KT * TRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hf = lane >> 5;
    int bh, q0;
    tile_of(L, bh, q0);
    const int h = bh & 7, b = bh >> 3;
    const float* base = qkv + (size_t)b * L * D3 + h * HD;
    const int q = q0 + wave * 32 + n, qc = q < L ? q : L - 1;
    f32x4 qf[4], gf[4];
    load_frag(qf, base + (size_t)qc * D3, hf);
    load_frag(gf, dout + ((size_t)b * L + qc) * D + h * HD, hf);
    const float lse2 = lse[(size_t)bh * L + qc], dl = delta[(size_t)bh * L + qc];
    const float c = LOG2E * INV_SQRT_HD;
    const uint32_t mrow = mask_row(key, bh, qc);
    f32x16 dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] = 0.f;

    Stage2 st;
    const int ntiles = (L + KT - 1) / KT;
    st.load(base + D, D3, base + 2 * D, D3, 0, L, tid);
    st.store(Ks[0], Vs[0], tid);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1, k0 = t * KT;
        if (t + 1 < ntiles) st.load(base + D, D3, base + 2 * D, D3, k0 + KT, L, tid);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            f32x16 s = rows_dot(Ks[buf], blk, n, hf, qf);              // S^T: rows = keys
            const f32x16 dp = rows_dot(Vs[buf], blk, n, hf, gf);       // dP^T
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = k0 + blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf;
                float p = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse2));
                if (j >= L) p = 0.f;
                float g = dp[r];
                if constexpr (DROP) g = mask_keep(key, mrow, j) ? g * rscale : 0.f;
                s[r] = p * (g - dl);                                   // dS^T
            }
            cols_acc(Ks[buf], blk, n, hf, s, dq);                      // dQ^T += K^T dS^T
        }
        if (t + 1 < ntiles) st.store(Ks[buf ^ 1], Vs[buf ^ 1], tid);
        __syncthreads();
    }
    if (q < L) store_grad(dqkv + ((size_t)b * L + q) * D3 + h * HD, dq, INV_SQRT_HD, hf);
}

// ---- dk | dv pass: a lane owns one key, the queries (q, dO, lse, delta) are streamed
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_train_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                                const float* __restrict__ delta, const float* __restrict__ dout,
                                                                float* __restrict__ dqkv, int L, MaskKey key, float rscale) {
    __shared__ __attribute__((aligned(16))) float Qs[2][KT * TRS];
    __shared__ __attribute__((aligned(16))) float Gs[2][KT * TRS];
    __shared__ __attribute__((aligned(16))) float Ls[2][2 * KT];       // [buffer][lse | delta] of the tile's queries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hf = lane >> 5;
    int bh, j0;
    tile_of(L, bh, j0);
    const int h = bh & 7, b = bh >> 3;
    const float* base = qkv + (size_t)b * L * D3 + h * HD;
    const float* gbase = dout + (size_t)b * L * D + h * HD;
    const float* stat = (tid < KT ? lse : delta) + (size_t)bh * L;      // threads 0 .. 127 stage the tile's lse and delta
    const int j = j0 + wave * 32 + n, jc = j < L ? j : L - 1;
    f32x4 kf[4], vf[4];
    load_frag(kf, base + (size_t)jc * D3 + D, hf);
    load_frag(vf, base + (size_t)jc * D3 + 2 * D, hf);
    const float c = LOG2E * INV_SQRT_HD;
    f32x16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = 0.f, dv[r] = 0.f;

    Stage2 st;
    float sreg = 0.f;
    const int ntiles = (L + KT - 1) / KT;
    auto load_stat = [&](int i0) {
        if (tid < 2 * KT) {
            const int i = i0 + (tid & (KT - 1));
            sreg = stat[i < L ? i : L - 1];
        }
    };
    st.load(base, D3, gbase, D, 0, L, tid);
    load_stat(0);
    st.store(Qs[0], Gs[0], tid);
    if (tid < 2 * KT) Ls[0][tid] = sreg;
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1, i0 = t * KT;
        if (t + 1 < ntiles) {
            st.load(base, D3, gbase, D, i0 + KT, L, tid);
            load_stat(i0 + KT);
        }
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            f32x16 s = rows_dot(Qs[buf], blk, n, hf, kf);              // S: rows = queries
            f32x16 dp = rows_dot(Gs[buf], blk, n, hf, vf);             // dP
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l2 = *reinterpret_cast<const f32x4*>(&Ls[buf][blk * 32 + 8 * g + 4 * hf]);
                const f32x4 dl = *reinterpret_cast<const f32x4*>(&Ls[buf][KT + blk * 32 + 8 * g + 4 * hf]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e, i = i0 + blk * 32 + 8 * g + 4 * hf + e;
                    float p = __builtin_amdgcn_exp2f(fmaf(s[r], c, -l2[e]));
                    if (i >= L) p = 0.f;
                    float pd = p;                                      // P' = keep P / (1 - p_drop)
                    if constexpr (DROP) pd = mask_keep(key, mask_row(key, bh, i), jc) ? p * rscale : 0.f;
                    s[r] = pd;
                    dp[r] = pd * dp[r] - p * dl[e];                    // dS
                }
            }
            cols_acc(Gs[buf], blk, n, hf, s, dv);                      // dV^T += dO^T P'
            cols_acc(Qs[buf], blk, n, hf, dp, dk);                     // dK^T += Q^T dS
        }
        if (t + 1 < ntiles) {
            st.store(Qs[buf ^ 1], Gs[buf ^ 1], tid);
            if (tid < 2 * KT) Ls[buf ^ 1][tid] = sreg;
        }
        __syncthreads();
    }
    if (j < L) {
        float* row = dqkv + ((size_t)b * L + j) * D3 + h * HD;
        store_grad(row + D, dk, INV_SQRT_HD, hf);
        store_grad(row + 2 * D, dv, 1.0f, hf);
    }
}

// keep[b, h, i, j] as bytes: what the forward and the backward regenerate, for the tests
__global__ __launch_bounds__(256) void attn_train_mask_kernel(uint8_t* __restrict__ keep, size_t total, int L, MaskKey key) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % L), i = (int)((idx / L) % L), bh = (int)(idx / ((size_t)L * L));
    keep[idx] = mask_keep(key, mask_row(key, bh, i), j) ? 1 : 0;
}

bool aligned16(const void* p) { return p && !(reinterpret_cast<uintptr_t>(p) & 15); }
bool valid_p(float p) { return p >= 0.f && p < 1.f; }                  // (NaN fails both)
// ceil(L / 128) * 8 * B workgroups of a pass, 0 where a launch does not take them
unsigned pass_grid(int B, int L) {
    const size_t n = (size_t)((L + QT - 1) / QT) * NH * B;
    return n > 0x7fffffff ? 0u : (unsigned)n;
}
MaskKey mask_key(float p, uint64_t seed) {
    return MaskKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)llround((double)p * 4294967296.0)};
}
int launched() { return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP; }

}  // namespace

}  // namespace clm

using namespace clm;

extern "C" int64_t clm_attn_train_workspace_bytes(int B, int L) {
    if (B < 1 || L < 1) return CLM_E_INVALID;
    return ((int64_t)B * NH * L * (int64_t)sizeof(float) + 15) & ~(int64_t)15;     // delta [B, 8, L]
}

extern "C" int clm_attn_train_forward(const float* qkv, float* out, float* lse, int B, int L, float dropout_p, uint64_t seed,
                                      void* stream) {
    if (B < 1 || L < 1 || !valid_p(dropout_p) || !aligned16(qkv) || !aligned16(out) || !aligned16(lse)) return CLM_E_INVALID;
    const unsigned grid = pass_grid(B, L);
    if (!grid) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const MaskKey key = mask_key(dropout_p, seed);
    if (dropout_p > 0.f)
        hipLaunchKernelGGL(attn_train_fwd_kernel<true>, dim3(grid), dim3(256), 0, st, qkv, out, lse, L, key, 1.0f / (1.0f - dropout_p));
    else
        hipLaunchKernelGGL(attn_train_fwd_kernel<false>, dim3(grid), dim3(256), 0, st, qkv, out, lse, L, key, 1.0f);
    return launched();
}

extern "C" int clm_attn_train_backward(const float* qkv, const float* out, const float* lse, const float* dout, float* dqkv,
                                       void* workspace, int B, int L, float dropout_p, uint64_t seed, void* stream) {
    if (B < 1 || L < 1 || !valid_p(dropout_p) || !aligned16(qkv) || !aligned16(out) || !aligned16(lse) || !aligned16(dout) ||
        !aligned16(dqkv) || !aligned16(workspace))
        return CLM_E_INVALID;
    const unsigned grid = pass_grid(B, L);
    const size_t nd = ((size_t)B * L * NH + 255) / 256;
    if (!grid || nd > 0x7fffffff) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const MaskKey key = mask_key(dropout_p, seed);
    float* delta = static_cast<float*>(workspace);
    const float rs = 1.0f / (1.0f - dropout_p);
    hipLaunchKernelGGL(attn_train_delta_kernel, dim3((unsigned)nd), dim3(256), 0, st, out, dout, delta, B, L);
    if (dropout_p > 0.f) {
        hipLaunchKernelGGL(attn_train_dq_kernel<true>, dim3(grid), dim3(256), 0, st, qkv, lse, delta, dout, dqkv, L, key, rs);
        hipLaunchKernelGGL(attn_train_dkv_kernel<true>, dim3(grid), dim3(256), 0, st, qkv, lse, delta, dout, dqkv, L, key, rs);
    } else {
        hipLaunchKernelGGL(attn_train_dq_kernel<false>, dim3(grid), dim3(256), 0, st, qkv, lse, delta, dout, dqkv, L, key, rs);
        hipLaunchKernelGGL(attn_train_dkv_kernel<false>, dim3(grid), dim3(256), 0, st, qkv, lse, delta, dout, dqkv, L, key, rs);
    }
    return launched();
}

extern "C" int clm_attn_train_mask(uint8_t* keep, int B, int L, float dropout_p, uint64_t seed, void* stream) {
    if (B < 1 || L < 1 || !valid_p(dropout_p) || !aligned16(keep)) return CLM_E_INVALID;
    const size_t total = (size_t)B * NH * L * L, nb = (total + 255) / 256;
    if (nb > 0x7fffffff) return CLM_E_INVALID;
    hipLaunchKernelGGL(attn_train_mask_kernel, dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep, total, L,
                       mask_key(dropout_p, seed));
    return launched();
}
