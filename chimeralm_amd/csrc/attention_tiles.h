// attention_tiles.h -- what the inference attention kernels (attention.hip) and the training op (attention_train.hip) share: the tiled
// online-softmax skeleton, the fp32 staging and the exact-fp32 arithmetic A32, with the geometry constants and the fp32 store.
// attention.hip's head comment describes the skeleton and what an arithmetic A is.
//
// Two things are here for the training forward and compile to nothing for the inference kernels:
//   * a per-tile hook on the probabilities, called between the row sum and pv(): hook.tile(p, bh, q, k0, hf) may rewrite the two
//     blocks' probabilities of this lane's query q (register r of block blk is key k0 + blk * 32 + (r & 3) + 8 (r >> 2) + 4 hf).
//     NoHook is empty;
//   * the running maximum m (of the raw, unscaled scores) and the softmax denominator lsum are returned next to inv = 1 / lsum.
#pragma once
#include "chimeralm_hip.h"
#include "gemm_common.h"

namespace clm {

namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
template <int N>
using fvec = float __attribute__((ext_vector_type(N)));
template <int N>
using hvec = _Float16 __attribute__((ext_vector_type(N)));

constexpr int HD = 32;            // head dim
constexpr int NH = D / HD;        // 8 heads
constexpr int QT = 128;           // queries per workgroup (4 waves x 32)
constexpr int KT = 64;            // keys per staged tile
// Tile row strides.  16-bit elements (A16, AX3): K rows padded to 80 bytes and V rows kept at 64 bytes so that the plain 16-byte
// reads of K and the transposing reads of V are both bank-conflict free (MI355X_MICROARCH.md "LDS": 4 x 16-lane groups for b128,
// 2 x 32 for the transposing read).  Floats (A32): the 16 rows of a ds_read_b128 group on 16 bank groups (K); rows 4 apart on
// banks + 32 (V, ds_read_b32).
constexpr int KRS = 40, VRS = 32;
constexpr int KRS32 = 36, VRS32 = 40;

// exchange between the two half-waves (lane ^ 32): one ds_bpermute per 64-key tile
__device__ __forceinline__ float half_max(float x) { return fmaxf(x, __shfl_xor(x, 32, 64)); }
__device__ __forceinline__ float half_sum(float x) { return x + __shfl_xor(x, 32, 64); }

struct NoHook {
    __device__ __forceinline__ void tile(f32x16 (&)[2], int, int, int, int) const {}
};

// The one text of the tile loop.  On return o = this lane's unnormalised O^T column (rows d = (r & 3) + 8 (r >> 2) + 4 hf), inv =
// 1 / its softmax denominator lsum, m = its largest raw score, and (b, h, q) = read, head and query of the lane; q >= L in the
// ragged last query tile.
template <class A, class Hook>
__device__ __forceinline__ void attention_tiles(A& a, const Hook& hook, const typename A::in_t* __restrict__ qkv, int L, f32x16& o,
                                                float& inv, float& m, float& lsum, int& b, int& h, int& q) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hf = lane >> 5;
    // Workgroup -> (query tile, head, read).  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with
    // its own L2: the query tiles of one (read, head) -- which all stream the same K / V -- are given ids that are congruent
    // modulo 8 so that they share one XCD's L2 (with the natural order every tile pulled its own copy of K / V through the fabric:
    // rocprofv3 FETCH_SIZE showed 2.2 GB per launch for 0.4 GB of qkv).
    const int ntq = (L + QT - 1) / QT;
    const int g = blockIdx.x, xcd = g & 7, slot = g >> 3;
    const int bh = (slot / ntq) * 8 + xcd;                          // B * 8 (read, head) pairs: always a multiple of 8
    const int q0 = (slot % ntq) * QT;
    h = bh & 7, b = bh >> 3;
    const typename A::in_t* base = qkv + (size_t)b * L * D3 + h * HD;   // row t: base + t * 768 ; q at +0, k at +256, v at +512
    const float c = 1.4426950408889634f * 0.17677669529663687f;      // log2(e) / sqrt(32)
    q = q0 + wave * 32 + n;
    a.load_q(base + (size_t)(q < L ? q : L - 1) * D3, hf);

#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    m = -INFINITY;                 // running maximum (shared by both halves)
    float l = 0.f;                 // this half's share of the running sum

    const int ntiles = (L + KT - 1) / KT;
    a.load_tile(base, 0, L, tid);
    a.store_tile(0, tid);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1, k0 = t * KT;
        if (t + 1 < ntiles) a.load_tile(base, k0 + KT, L, tid);       // in flight under the block below
        // ---- S^T = K Q^T for the 64 keys of the tile: two 32-key blocks
        f32x16 s[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) s[blk] = a.scores(buf, blk, n, hf);
        if (k0 + KT > L) {                                             // last tile: keys beyond the read
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf >= L) s[blk][r] = -INFINITY;
        }
        // ---- online softmax: this lane's query, 32 of the 64 keys here, the other 32 in the partner half-wave
        float mx = s[0][0];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[blk][r]);
        mx = half_max(mx);
        const float m_new = fmaxf(m, mx);                              // finite: key k0 is always valid
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * c);   // 0 on the first tile (m = -inf)
        const float mc = m_new * c;
        float psum = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[blk][r] = __builtin_amdgcn_exp2f(fmaf(s[blk][r], c, -mc));
                psum += s[blk][r];
            }
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
        hook.tile(s, bh, q, k0, hf);                                   // (training: the dropout keep mask; l sums the undropped p)
        a.pv(buf, s, o, lane, n, hf);                                  // ---- O^T += V^T P^T
        if (t + 1 < ntiles) a.store_tile(buf ^ 1, tid);                // the other buffer was last read in trip t - 1
        __syncthreads();
    }
    lsum = half_sum(l);
    inv = 1.0f / lsum;
}

// ---- fp32 staging shared by the two exact arithmetics: thread -> (key row, 4-float piece) x 2 of the K and of the V tile
struct StageF32 {
    using in_t = float;
    f32x4 kreg[2], vreg[2];
    __device__ __forceinline__ void load_tile(const float* base, int k0, int L, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * 256, j = e >> 3, d4 = e & 7;
            const int key = k0 + j < L ? k0 + j : L - 1;                // clamped; the score mask removes the clones
            const float* p = base + (size_t)key * D3 + 4 * d4;
            kreg[i] = *reinterpret_cast<const f32x4*>(p + D);
            vreg[i] = *reinterpret_cast<const f32x4*>(p + 2 * D);
        }
    }
};

// ---- exact fp32: v_mfma_f32_32x32x2_f32, 16 MFMAs per 32-key block for the scores and 16 for P V: per 64-key tile 64 MFMAs of 64
// cycles next to ~900 cycles of softmax VALU -- MFMA-bound.  Accumulator register t of a block IS the B operand of step t of
// O^T = V^T P^T, with the A operand read from the V row of the key that register holds (lanes 0-31 feed key (t & 3) + 8 (t >> 2),
// lanes 32-63 that key + 4): V rows are stored in key order.  38 KiB of LDS.
struct A32 : StageF32 {
    float *Ks, *Vs;                // [2][KT * KRS32], [2][KT * VRS32]
    f32x4 qf[4];                   // Q^T as B operand: d = 8 s + 4 hf + 0..3

    __device__ __forceinline__ void load_q(const float* row, int hf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const f32x4*>(row + 4 * hf + 8 * s);
    }
    __device__ __forceinline__ void store_tile(int buf, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * 256, j = e >> 3, d4 = e & 7;
            *reinterpret_cast<f32x4*>(&Ks[buf * KT * KRS32 + j * KRS32 + 4 * d4]) = kreg[i];
            *reinterpret_cast<f32x4*>(&Vs[buf * KT * VRS32 + j * VRS32 + 4 * d4]) = vreg[i];
        }
    }
    __device__ __forceinline__ f32x16 scores(int buf, int blk, int n, int hf) const {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const float* kp = &Ks[buf * KT * KRS32 + (blk * 32 + n) * KRS32 + 4 * hf];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const f32x4 kf = *reinterpret_cast<const f32x4*>(kp + 8 * st);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[st][j], s, 0, 0, 0);
        }
        return s;
    }
    __device__ __forceinline__ void pv(int buf, const f32x16 (&p)[2], f32x16& o, int lane, int n, int hf) const {
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const float* vp = &Vs[buf * KT * VRS32 + (blk * 32 + 4 * hf) * VRS32 + n];
#pragma unroll
            for (int t = 0; t < 16; ++t)
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[((t & 3) + 8 * (t >> 2)) * VRS32], p[blk][t], o, 0, 0, 0);
        }
    }
};

// output of the exact kernels: lane (query n, half hf) holds d = (r & 3) + 8 (r >> 2) + 4 hf
__device__ __forceinline__ void store_f32(float* __restrict__ out, int L, const f32x16& o, float inv, int b, int h, int q) {
    if (q >= L) return;
    const int hf = (threadIdx.x >> 5) & 1;
    float* op = out + ((size_t)b * L + q) * D + h * HD + 4 * hf;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
        *reinterpret_cast<float4*>(op + 8 * gq) = make_float4(o[4 * gq + 0] * inv, o[4 * gq + 1] * inv, o[4 * gq + 2] * inv, o[4 * gq + 3] * inv);
}

}  // namespace

}  // namespace clm
