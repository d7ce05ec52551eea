// attn_weights.hip -- the pooling softmax as an OUTPUT: per-base attention weights, their masses and the top-k peaks of every read.
//
// Reference arithmetic:
//   BinarySequenceClassifier.forward     /root/reference/chimeralm/models/components/hyena.py:117-130
//     attention_weights = softmax(self.attention(x), dim=1) over ALL L positions ([PAD] and [SEP] included; the mask is always
//     None: hyena.py:256), kept when save_attention is set (hyena.py:129-130)
//   notebooks/attention.ipynb            find_attention_peaks(weights, top_k=10) = np.argsort(weights)[-top_k:][::-1] on the
//     read's bases (weights[:-1] strips [SEP]; pads are stripped by the caller)
//
// One workgroup per read, behind stage_head on the forward's stream.  The read's scores (fp32 [L], <= 32,770 x 4 B = 128 KiB) cross
// HBM once, into LDS; the maximum, the sum, the normalisation and the selection rounds run from LDS and registers.  Three kernels
// (256 / 512 / 1024 threads with 8 / 33 / 129 KiB of LDS) so that short reads do not pay for the long reads' footprint.
// No atomics, fixed reduction order: bitwise the same from run to run.  Sums are carried in fp64 (their rounding then does not
// show next to the fp32 exp).
#include <climits>

#include "chimeralm_hip.h"
#include "clm_common.h"

namespace clm {

namespace {

constexpr int SEP_ID = 1;         // [SEP] of the reference's tokenizer (the last token of every read)
constexpr int ATTN_MAXW = 16;     // waves of the largest workgroup

// fixed-order wave reductions (xor butterflies: every lane ends with the same bits)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
// the larger weight; equal weights: the lower position.  A total order, so the winner does not depend on the reduction's shape
__device__ __forceinline__ bool peak_before(float va, int pa, float vb, int pb) { return va > vb || (va == vb && pa < pb); }

// scores [Bc][L] and ids8 [Bc][Lp] of the chunk; the outputs start at the chunk's first read (the caller offsets them).
// Dynamic LDS: at least L floats.  weights / summary may be null (not both); peak_pos / peak_w go with summary.
template <int NT>
__global__ __launch_bounds__(NT) void attn_weights_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ ids8,
                                                          int L, int Lp, float* __restrict__ weights, int64_t w_stride,
                                                          clm_attn_summary* __restrict__ summary, int* __restrict__ peak_pos,
                                                          float* __restrict__ peak_w, int top_k) {
    constexpr int NW = NT / 64;
    extern __shared__ float w[];                             // [L]: scores, then exp(s - max), then the weights
    __shared__ float red_f[2][ATTN_MAXW];
    __shared__ int red_i[2][ATTN_MAXW];
    __shared__ int red_bad[ATTN_MAXW];
    __shared__ double red_d[3][ATTN_MAXW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* const s = scores + (size_t)b * L;
    const unsigned char* const ids = ids8 + (size_t)b * Lp;

    // 1: scores -> LDS (their one trip through HBM); maximum, NaN / inf, end of the leading run of [PAD]
    float m = -INFINITY;
    int bad = 0, first = L;
    for (int t = tid; t < L; t += NT) {
        const float v = s[t];
        w[t] = v;
        m = fmaxf(m, v);
        bad |= !(fabsf(v) <= 3.0e38f);
        if (ids[t] != PAD_ID) first = min(first, t);
    }
    m = wave_max(m);
    first = wave_min_i(first);
    bad = __any(bad);
    if (lane == 0) { red_f[0][wave] = m; red_i[0][wave] = first; red_bad[wave] = bad; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; ++i) { m = fmaxf(m, red_f[0][i]); first = min(first, red_i[0][i]); bad |= red_bad[i]; }
    const int n_pad = first;
    const int has_sep = ids[L - 1] == SEP_ID;
    const int n_bases = max(0, L - n_pad - has_sep);

    // 2: exp(s - max) and its sum (every thread works on the elements it wrote itself: no barrier in between)
    double sum = 0.0;
    for (int t = tid; t < L; t += NT) {
        const float e = expf(w[t] - m);
        w[t] = e;
        sum += (double)e;
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) red_d[0][wave] = sum;
    __syncthreads();
    sum = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) sum += red_d[0][i];
    const float inv = (float)(1.0 / sum);

    // 3: the weights, to LDS and (when asked for) to the caller's rows; masses of the [PAD] run and of the bases
    float* const wout = weights ? weights + (size_t)b * w_stride : nullptr;
    double pad_m = 0.0, base_m = 0.0;
    for (int t = tid; t < L; t += NT) {
        const float v = w[t] * inv;
        w[t] = v;
        if (wout) wout[t] = v;
        if (t < n_pad) pad_m += (double)v;
        else if (t < n_pad + n_bases) base_m += (double)v;
    }
    if (!summary) return;                                    // (uniform)
    pad_m = wave_sum_f64(pad_m);
    base_m = wave_sum_f64(base_m);
    if (lane == 0) { red_d[1][wave] = pad_m; red_d[2][wave] = base_m; }
    __syncthreads();                                         // (w[L - 1] is written as well)
    pad_m = 0.0; base_m = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { pad_m += red_d[1][i]; base_m += red_d[2][i]; }
    const int n_peaks = bad ? 0 : min(top_k, n_bases);
    if (tid == 0) {
        const float nan = __builtin_nanf("");
        clm_attn_summary r;
        r.n_pad = n_pad; r.n_bases = n_bases; r.has_sep = has_sep; r.n_peaks = n_peaks;
        r.pad_weight = bad ? nan : (float)pad_m;
        r.sep_weight = bad ? nan : (has_sep ? w[L - 1] : 0.f);
        r.base_weight = bad ? nan : (float)base_m;
        r.reserved = 0;
        summary[b] = r;
    }
    if (tid < top_k && tid >= n_peaks) {                     // slots no peak fills (top_k <= 32 < NT)
        peak_pos[(size_t)b * top_k + tid] = -1;
        peak_w[(size_t)b * top_k + tid] = 0.f;
    }
    if (n_peaks == 0) return;                                // (uniform)

    // 4: n_peaks selection rounds.  Every thread keeps the best of its own elements; a round finds the best of all, and only the
    // thread that owned it looks through its elements again (the winner is struck out in LDS: weights are >= 0)
    const int t_end = n_pad + n_bases;
    int t0 = tid + (n_pad / NT) * NT;                        // this thread's first base position
    if (t0 < n_pad) t0 += NT;
    float bv = -1.f;
    int bp = INT_MAX;
    for (int t = t0; t < t_end; t += NT)
        if (w[t] > bv) { bv = w[t]; bp = t; }                // (ascending t, strict: the lower position wins a tie)
    for (int k = 0; k < n_peaks; ++k) {
        float v = bv;
        int p = bp;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int op = __shfl_xor(p, o, 64);
            if (peak_before(ov, op, v, p)) { v = ov; p = op; }
        }
        const int buf = k & 1;                               // (two buffers: one barrier per round)
        if (lane == 0) { red_f[buf][wave] = v; red_i[buf][wave] = p; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (peak_before(red_f[buf][i], red_i[buf][i], v, p)) { v = red_f[buf][i]; p = red_i[buf][i]; }
        if (tid == 0) {
            peak_pos[(size_t)b * top_k + k] = p - n_pad;
            peak_w[(size_t)b * top_k + k] = v;
        }
        if (p == bp) {                                       // mine: strike it out, find my next best
            w[p] = -1.f;
            bv = -1.f;
            bp = INT_MAX;
            for (int t = t0; t < t_end; t += NT)
                if (w[t] > bv) { bv = w[t]; bp = t; }
        }
    }
}

}  // namespace

void launch_attn_weights(const float* scores, const unsigned char* ids8, int Bc, int L, int Lp, float* weights, int64_t w_stride,
                         clm_attn_summary* summary, int* peak_pos, float* peak_w, int top_k, hipStream_t st) {
    // one LDS size per kernel (launch_lds): the class's capacity, not L
    if (L <= 2048)
        launch_lds<attn_weights_kernel<256>>(dim3(Bc), dim3(256), (size_t)2048 * 4, st, scores, ids8, L, Lp, weights, w_stride, summary,
                                             peak_pos, peak_w, top_k);
    else if (L <= 8448)
        launch_lds<attn_weights_kernel<512>>(dim3(Bc), dim3(512), (size_t)8448 * 4, st, scores, ids8, L, Lp, weights, w_stride, summary,
                                             peak_pos, peak_w, top_k);
    else
        launch_lds<attn_weights_kernel<1024>>(dim3(Bc), dim3(1024), (size_t)ATTN_MAX_L * 4, st, scores, ids8, L, Lp, weights, w_stride,
                                              summary, peak_pos, peak_w, top_k);
}

}  // namespace clm
