// attention.hip -- multi-head self-attention forward for the SequenceCNNTransformer encoder: ONE
// tiled online-softmax skeleton (attention_tiles) and the three MFMA arithmetics that run on it -- 16 bit (fp16 / bf16, and fp16c's
// two-plane output), exact fp32, and fp16x3.
//
// Reference arithmetic: nn.TransformerEncoderLayer's self-attention as the reference constructs it
//   /root/reference/chimeralm/models/components/transformer.py:64-68,98   (d_model 256, nhead 8 -> head dim 32, batch_first,
//   no attention mask and no key-padding mask: every position attends to every position of its read)
//       a[b, i, h, :] = sum_j softmax_j(q[b,i,h,:] . k[b,j,h,:] / sqrt(32)) v[b, j, h, :]
// with q | k | v the three 256-wide thirds of the in_proj output (in_proj_weight [768, 256] is laid out q, k, v).
//
// Shape of the problem on MI355X: head dim 32 makes the softmax, not the matrix products, the bound -- per 32 x 32 block of
// scores a wave issues 4 16-bit MFMAs (128 cycles of pipe) and ~450 cycles of VALU (exp2 at quarter rate).  So the skeleton is
// built around a cheap softmax:
//   * scores are computed TRANSPOSED, S^T = K Q^T (rows = keys, columns = queries): in the 32x32 accumulator layout a lane then
//     owns ONE query (column l & 31) and 16 of its 32 keys in registers, so the row maximum / row sum of the softmax are
//     register reductions plus one exchange between the two half-waves (lane ^ 32) -- no 32-lane shuffle trees;
//   * exp2(s*c - m*c) with c = log2(e)/sqrt(32): one FMA + one v_exp_f32 per score, in place in the score accumulators;
//   * P^T never leaves the registers: the accumulator registers of S^T ARE (converted, split, or as they are) the B operand of
//     O^T = V^T P^T, because the key index, being the reduction index, may be paired freely as long as V's rows are paired the
//     same way -- each arithmetic's pv() says how it pairs them;
//   * 256-thread workgroups (4 waves x 32 queries), 64-key tiles double-buffered in LDS, the next tile's global loads in flight
//     under the current tile's arithmetic: several workgroups per CU hide the exp latency of each other.
// Online softmax (running maximum m, running sum l, accumulator rescaled when m grows) over the key tiles; keys beyond L are
// masked to -inf in the last tile; fp32 statistics and accumulation in every arithmetic.
//
// An arithmetic A is a plain struct of registers and LDS pointers:
//   in_t                                element type of qkv
//   load_q(row, hf)                     Q^T fragments of this lane's query (row = its q, this head) into registers
//   load_tile(base, k0, L, tid)         keys k0 .. k0 + 63 (clamped to L - 1) of K and V from global memory into registers
//   store_tile(buf, tid)                ... from there into LDS buffer buf
//   scores(buf, blk, n, hf) -> f32x16   S^T of the 32-key block blk
//   pv(buf, p, o, lane, n, hf)          o += V^T P^T, p = the two blocks' fp32 probabilities in accumulator layout: register r of
//                                       block blk is key blk * 32 + (r & 3) + 8 (r >> 2) + 4 hf of the tile
//
// The skeleton, the fp32 staging, A32 and the fp32 store live in attention_tiles.h, which the training op (attention_train.hip) shares.
#include "attention_tiles.h"

namespace clm {

namespace {

using s16x8 = short __attribute__((ext_vector_type(8)));
using v4i16 = short __attribute__((ext_vector_type(4)));
typedef v4i16 __attribute__((address_space(3))) * lds_v4i16_ptr;


// A16 / AX3: the accumulator registers 8 s .. 8 s + 7 of a block are, as B operand of a K = 16 MFMA step, its 16 keys with bits 2 and
// 3 of the key index swapped.  V rows are simply stored in that order when the tile is staged: v_row(k) holds key k (k < KT) ...
__device__ __forceinline__ int v_row(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }
// ... and the V^T fragment of a step comes from the [key row][d] tile with two transposing reads (ds_read_tr16_b64), rows 4 apart
template <class F, class T>
__device__ __forceinline__ F vt_frag(const T* p0) {
    const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr)(p0));
    const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr)(p0 + 4 * VRS));
    const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(F, both);
}


// ---- 16 bit: fp16 / bf16 operands, v_mfma_f32_32x32x16; 4 MFMAs per 32-key block for the scores and 4 for P V.  18 KiB of LDS.
template <int PREC>
struct A16 {
    using in_t = typename CT<PREC>::elem;
    in_t *Ks, *Vs;                 // [2][KT * KRS], [2][KT * VRS]
    u16x8 qf[2];                   // Q^T as B operand, both k-steps: lane (query n, half hf) holds q[d = 16 s + 8 hf + 0..7]
    uint4 kreg, vreg;              // staging: thread -> (key row tid >> 2, 16-byte piece tid & 3) of the K and of the V tile

    __device__ __forceinline__ void load_q(const in_t* row, int hf) {
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const u16x8*>(row + 16 * s + 8 * hf);
    }
    __device__ __forceinline__ void load_tile(const in_t* base, int k0, int L, int tid) {
        const int sk = tid >> 2, sp = tid & 3;
        const int key = k0 + sk < L ? k0 + sk : L - 1;                // clamped; the score mask removes the clones
        const in_t* p = base + (size_t)key * D3 + 8 * sp;
        kreg = *reinterpret_cast<const uint4*>(p + D);
        vreg = *reinterpret_cast<const uint4*>(p + 2 * D);
    }
    __device__ __forceinline__ void store_tile(int buf, int tid) {
        const int sk = tid >> 2, sp = tid & 3;
        *reinterpret_cast<uint4*>(&Ks[buf * KT * KRS + sk * KRS + 8 * sp]) = kreg;
        *reinterpret_cast<uint4*>(&Vs[buf * KT * VRS + v_row(sk) * VRS + 8 * sp]) = vreg;
    }
    __device__ __forceinline__ f32x16 scores(int buf, int blk, int n, int hf) const {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const u16x8 kf = *reinterpret_cast<const u16x8*>(&Ks[buf * KT * KRS + (blk * 32 + n) * KRS + 16 * ks + 8 * hf]);
            s = mfma<PREC>(kf, qf[ks], s);
        }
        return s;
    }
    __device__ __forceinline__ void pv(int buf, const f32x16 (&p)[2], f32x16& o, int lane, int n, int hf) const {
        const int li = lane & 15, g1 = (lane >> 4) & 1, q4 = li >> 2, p4 = li & 3;
        const in_t* vb = &Vs[buf * KT * VRS + (8 * hf + q4) * VRS + 16 * g1 + 4 * p4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u16x8 pf;                                              // P^T as B operand of this 16-key step
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = from_float<in_t>(p[blk][8 * ks + j]).bits;
                o = mfma<PREC>(vt_frag<u16x8>(vb + (blk * 32 + ks * 16) * VRS), pf, o);
            }
    }
};


// ---- fp16x3: every operand as two halfs (hi = fp16(x), lo = fp16(x - hi)) and three fp16 MFMAs per product (hi hi, lo hi, hi lo):
// 12 MFMAs per 32-key block for the scores and 12 for P V.  q / k / v arrive as fp32 and are split on their way into registers / LDS,
// the probabilities per 16-key step, immediately before that step's MFMAs.  Operand layouts, strides, the V-row permutation and the
// transposing V reads are A16's, with a hi and a lo plane of every tile: 36 KiB of LDS.
struct AX3 : StageF32 {
    _Float16 *Ks, *Vs;             // [2][2][KT * KRS], [2][2][KT * VRS]: [buffer][hi | lo]
    hvec<8> qh[2], ql[2];          // Q^T as B operand: d = 16 s + 8 hf + 0..7

    template <int N>
    static __device__ __forceinline__ fvec<N> clamp(fvec<N> v) {      // (beyond fp16's range: saturate, never inf -- tail32.hip split4)
        fvec<N> r;
#pragma unroll
        for (int e = 0; e < N; ++e) r[e] = __builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
        return r;
    }
    template <int N>
    static __device__ __forceinline__ void split(fvec<N> v, hvec<N>& hi, hvec<N>& lo) {
        hi = __builtin_convertvector(clamp<N>(v), hvec<N>);
        lo = __builtin_convertvector(clamp<N>(v - __builtin_convertvector(hi, fvec<N>)), hvec<N>);
    }
    static __device__ __forceinline__ f32x16 mm(hvec<8> a, hvec<8> b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }

    __device__ __forceinline__ void load_q(const float* row, int hf) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + 8 * hf + 16 * s), y = *reinterpret_cast<const f32x4*>(row + 8 * hf + 16 * s + 4);
            split<8>(fvec<8>{x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]}, qh[s], ql[s]);
        }
    }
    __device__ __forceinline__ void store_tile(int buf, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + i * 256, j = e >> 3, d4 = e & 7;
            hvec<4> kh, kl, vh, vl;
            split<4>(kreg[i], kh, kl);
            split<4>(vreg[i], vh, vl);
            _Float16* kp = &Ks[buf * 2 * KT * KRS + j * KRS + 4 * d4];
            _Float16* vp = &Vs[buf * 2 * KT * VRS + v_row(j) * VRS + 4 * d4];
            *reinterpret_cast<hvec<4>*>(kp) = kh;
            *reinterpret_cast<hvec<4>*>(kp + KT * KRS) = kl;
            *reinterpret_cast<hvec<4>*>(vp) = vh;
            *reinterpret_cast<hvec<4>*>(vp + KT * VRS) = vl;
        }
    }
    __device__ __forceinline__ f32x16 scores(int buf, int blk, int n, int hf) const {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const _Float16* kp = &Ks[buf * 2 * KT * KRS + (blk * 32 + n) * KRS + 16 * ks + 8 * hf];
            const hvec<8> kh = *reinterpret_cast<const hvec<8>*>(kp), kl = *reinterpret_cast<const hvec<8>*>(kp + KT * KRS);
            s = mm(kh, qh[ks], s);
            s = mm(kl, qh[ks], s);
            s = mm(kh, ql[ks], s);
        }
        return s;
    }
    __device__ __forceinline__ void pv(int buf, const f32x16 (&p)[2], f32x16& o, int lane, int n, int hf) const {
        const int li = lane & 15, g1 = (lane >> 4) & 1, q4 = li >> 2, p4 = li & 3;
        const _Float16* vb = &Vs[buf * 2 * KT * VRS + (8 * hf + q4) * VRS + 16 * g1 + 4 * p4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fvec<8> pp;
#pragma unroll
                for (int j = 0; j < 8; ++j) pp[j] = p[blk][8 * ks + j];
                hvec<8> ph, pl;                                        // P^T as B operand of this 16-key step, hi and lo halfs
                split<8>(pp, ph, pl);
                const _Float16* p0 = vb + (blk * 32 + ks * 16) * VRS;
                const hvec<8> vh = vt_frag<hvec<8>>(p0), vl = vt_frag<hvec<8>>(p0 + KT * VRS);
                o = mm(vh, ph, o);
                o = mm(vl, ph, o);
                o = mm(vh, pl, o);
            }
    }
};


}  // namespace

// HILO (round 3, the transformer's fp16c mode): the output leaves as TWO 16-bit planes, out[0] = fp16(64 a) and out[1] =
// fp16(64 a - out[0]), `plane` elements apart.  The attention output is close to the same vector at every position of a read
// (an average of v over all keys), so its rounding to 16 bits is the one activation rounding of this net that does NOT average
// out in the pooling: measured on the CPU (tests/tf_error_probe.py) it alone moves the logits by 2-4e-3 where every other
// operand's rounding stays below 1e-3.  The factor 64 (exact) keeps the lo plane out of fp16's subnormal range; out_proj
// multiplies both planes by the same weights and scales its accumulators by 1/64 (tf_model.hip, enc_ffn16_kernel).
constexpr float ATT_HILO_SCALE = 64.0f;

template <int PREC, bool HILO = false>
__global__ __launch_bounds__(256, 4) void attention_fwd_kernel(const typename CT<PREC>::elem* __restrict__ qkv,
                                                            typename CT<PREC>::elem* __restrict__ out, int L, size_t plane) {
    using elem = typename CT<PREC>::elem;
    __shared__ __attribute__((aligned(16))) elem Ks[2][KT * KRS];
    __shared__ __attribute__((aligned(16))) elem Vs[2][KT * VRS];
    A16<PREC> a;
    a.Ks = &Ks[0][0], a.Vs = &Vs[0][0];
    f32x16 o;                      // O^T: rows d, column = this lane's query
    float inv, m, lsum;
    int b, h, q;
    attention_tiles(a, NoHook{}, qkv, L, o, inv, m, lsum, b, h, q);
    // ---- normalise and store: lane (query n, half hf) holds d = (r & 3) + 8 (r >> 2) + 4 hf
    const int hf = (threadIdx.x >> 5) & 1;
    if (q < L) {
        elem* op = out + ((size_t)b * L + q) * D + h * HD + 4 * hf;
        const float sc = HILO ? inv * ATT_HILO_SCALE : inv;
        if constexpr (HILO) {
            // One fp32 product x, one hi = fp16(x), and lo the rounding of their exact difference.  x is made opaque to the compiler:
            // under -ffp-contract=fast it rounded o * sc to fp16 twice, once through fp32 for the stored hi (v_cvt_pk_f16_f32) and
            // once directly from the exact product for the hi that lo is measured against (v_fma_mixlo_f16).  Where the two
            // roundings fell on different sides of an fp16 midpoint the pair (hi, lo) was a whole ulp(hi) off: 131.0 - 0.0625
            // stored for 131.0625 (tests/test_gpu_attention16.py).
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u16x4 pk, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = o[4 * g + e] * sc;
                    asm("" : "+v"(x));
                    const elem hi = from_float<elem>(x);
                    pk[e] = hi.bits;
                    pl[e] = from_float<elem>(x - to_float(hi)).bits;
                }
                *reinterpret_cast<u16x4*>(op + 8 * g) = pk;
                *reinterpret_cast<u16x4*>(op + plane + 8 * g) = pl;
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const elem e0 = from_float<elem>(o[4 * g + 0] * sc), e1 = from_float<elem>(o[4 * g + 1] * sc),
                           e2 = from_float<elem>(o[4 * g + 2] * sc), e3 = from_float<elem>(o[4 * g + 3] * sc);
                u16x4 pk = {e0.bits, e1.bits, e2.bits, e3.bits};
                *reinterpret_cast<u16x4*>(op + 8 * g) = pk;
            }
        }
    }
}

__global__ __launch_bounds__(256, 4) void attention32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int L) {
    __shared__ __attribute__((aligned(16))) float Ks[2][KT * KRS32];
    __shared__ __attribute__((aligned(16))) float Vs[2][KT * VRS32];
    A32 a;
    a.Ks = &Ks[0][0], a.Vs = &Vs[0][0];
    f32x16 o;
    float inv, m, lsum;
    int b, h, q;
    attention_tiles(a, NoHook{}, qkv, L, o, inv, m, lsum, b, h, q);
    store_f32(out, L, o, inv, b, h, q);
}

__global__ __launch_bounds__(256, 3) void attention_x3_kernel(const float* __restrict__ qkv, float* __restrict__ out, int L) {
    __shared__ __attribute__((aligned(16))) _Float16 Ks[2][2][KT * KRS];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[2][2][KT * VRS];
    AX3 a;
    a.Ks = &Ks[0][0][0], a.Vs = &Vs[0][0][0];
    f32x16 o;
    float inv, m, lsum;
    int b, h, q;
    attention_tiles(a, NoHook{}, qkv, L, o, inv, m, lsum, b, h, q);
    store_f32(out, L, o, inv, b, h, q);
}

// grid of every launch here: ceil(L / QT) query tiles x 8 heads x B reads; false where that is more than a launch takes
static bool attention_grid(int B, int L, dim3& grid) {
    static_assert(NH == 8, "the workgroup -> XCD mapping assumes 8 heads");
    const size_t n = (size_t)((L + QT - 1) / QT) * NH * B;
    if (n > 0x7fffffff) return false;
    grid = dim3((unsigned)n);
    return true;
}

bool launch_attention_fwd(int prec, const void* qkv, void* out, int B, int L, hipStream_t st, bool hilo) {
    dim3 grid, block(256);
    if (!attention_grid(B, L, grid)) return false;
    const size_t plane = (size_t)B * L * D;
    if (prec == PREC_BF16)
        hipLaunchKernelGGL(attention_fwd_kernel<PREC_BF16>, grid, block, 0, st, (const bf16_t*)qkv, (bf16_t*)out, L, plane);
    else if (hilo)
        hipLaunchKernelGGL((attention_fwd_kernel<PREC_F16, true>), grid, block, 0, st, (const f16_t*)qkv, (f16_t*)out, L, plane);
    else
        hipLaunchKernelGGL(attention_fwd_kernel<PREC_F16>, grid, block, 0, st, (const f16_t*)qkv, (f16_t*)out, L, plane);
    return true;
}

bool launch_attention_exact(bool x3, const float* qkv, float* out, int B, int L, hipStream_t st) {
    dim3 grid, block(256);
    if (!attention_grid(B, L, grid)) return false;
    if (x3) hipLaunchKernelGGL(attention_x3_kernel, grid, block, 0, st, qkv, out, L);
    else hipLaunchKernelGGL(attention32_kernel, grid, block, 0, st, qkv, out, L);
    return true;
}

}  // namespace clm

// ---- C ABI (include/chimeralm_hip.h): the attention launches on their own, for the tests that hold the kernels to an fp64
// softmax(q k^T / sqrt(32)) v at shapes and score patterns a whole-model bound cannot resolve
extern "C" int clm_attention_fwd(const void* qkv, void* out, int B, int L, int precision, void* stream) {
    if (!qkv || !out || B < 1 || L < 1) return CLM_E_INVALID;
    if (precision != CLM_PREC_F16 && precision != CLM_PREC_BF16 && precision != CLM_PREC_F16C) return CLM_E_INVALID;
    // the kernel reads qkv in 16-byte pieces and writes out in 8-byte ones: refuse what it cannot address, before any launch
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return CLM_E_INVALID;
    // CLM_PREC_F16C: the transformer's fp16c attention, fp16 operands and the two-plane HILO output (as tf_model.hip launches it)
    if (!clm::launch_attention_fwd(precision == CLM_PREC_BF16 ? clm::PREC_BF16 : clm::PREC_F16, qkv, out, B, L,
                                   reinterpret_cast<hipStream_t>(stream), precision == CLM_PREC_F16C))
        return CLM_E_INVALID;
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}

extern "C" int clm_attention_exact_fwd(const float* qkv, float* out, int B, int L, int precision, void* stream) {
    if (!qkv || !out || B < 1 || L < 1 || (precision != CLM_PREC_F32 && precision != CLM_PREC_F16X3)) return CLM_E_INVALID;
    // the kernels read qkv and write out as float4
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return CLM_E_INVALID;
    if (!clm::launch_attention_exact(precision == CLM_PREC_F16X3, qkv, out, B, L, reinterpret_cast<hipStream_t>(stream))) return CLM_E_INVALID;
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}
