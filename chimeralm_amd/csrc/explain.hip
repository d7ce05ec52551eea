// explain.hip -- in-silico mutagenesis on MI355X: the mutant plan, three kernels, a handle and the C ABI (clm_explain_*).
//
// Reference arithmetic:
//   Mamba2Analyzer.get_position_importance     /root/reference/chimeralm/explain/motif.py:64-82
//     for every position i: the read with base i replaced by "N" through the model again; importance[i] = |p1(read) - p1(mutant)|
//     with p1 = softmax(logits)[1].  One forward of one read per position, each followed by .item() (a host wait).
//
// Here the scan sits above the `net` boundary and serves every net: the host enumerates the mutants of a read once (clm_explain_plan),
// the mutant rows of a batch are written on the device in the uint8 form every net's forward takes (explain_rows_kernel), the
// forward is the net's own, and one small kernel behind it turns the batch's logits into signed differences at the plan's slots
// (explain_scores_kernel).  When every batch has gone by, one workgroup folds the windows into per-base importance and selects the
// largest bases (explain_reduce_kernel: working values in LDS, the total order of attn_weights.hip).  Everything is queued on the
// caller's stream; no atomics, fixed reduction orders: bitwise the same from run to run.
#include <climits>
#include <cmath>
#include <string>

#include "handle_host.h"

namespace clm {
namespace explain {

constexpr int SEP_ID = 1, BASE_A = 7, BASE_N = 11;         // A, C, G, T, N = 7 ... 11 (the reference's tokenizer)
constexpr int ROWS_THREADS = 256;              // explain_rows_kernel: one 16-byte chunk of one row per thread
constexpr int SCORE_THREADS = 256, SCORE_WAVES = SCORE_THREADS / 64;
constexpr int MAX_BASES = 32768;               // bases of one read (the tokenizer's longest read); importance [n_bases] fits LDS
constexpr int RED_MAXW = 16;                   // waves of the largest reduce workgroup

// ---- mutant rows --------------------------------------------------------------------------------------------------------------
// Row r of `out` is mutant m0 + r: the read's ids with bases [start, min(start + window, n_bases)) replaced by the plan's substitute.
// A thread owns 16 consecutive tokens of one row and stores them once (the bytes between L and the next multiple of 16 are
// written as 0; row_stride is a multiple of 16 that holds them).  [SEP] at L - 1 = n_bases lies outside every window.
__global__ __launch_bounds__(ROWS_THREADS) void explain_rows_kernel(const unsigned char* __restrict__ ids, int L, int window,
                                                                    const clm_explain_mutant* __restrict__ plan, int m0,
                                                                    unsigned char* __restrict__ out, int64_t row_stride) {
    const int chunk = (int)(blockIdx.x * ROWS_THREADS + threadIdx.x);
    const int t0 = chunk * 16;
    if (t0 >= L) return;
    const clm_explain_mutant mu = plan[m0 + (int)blockIdx.y];
    const int lo = mu.start, hi = min(mu.start + window, L - 1);
    unsigned w[4];
    if (t0 + 16 <= L) {
        const uint4 v = *reinterpret_cast<const uint4*>(ids + t0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int t = t0 + 4 * i + b;
                if (t < L) w[i] |= (unsigned)ids[t] << (8 * b);
            }
        }
    }
    if (lo < t0 + 16 && hi > t0) {               // (the window meets this chunk)
        const unsigned sub = (unsigned)(mu.sub & 0xFF) * 0x01010101u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned mask = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int t = t0 + 4 * i + b;
                if (t >= lo && t < hi) mask |= 0xFFu << (8 * b);
            }
            w[i] = (w[i] & ~mask) | (sub & mask);
        }
    }
    *reinterpret_cast<uint4*>(out + (size_t)blockIdx.y * row_stride + t0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- scores -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// p1 = softmax(l)[1] in double from the fp32 logits, the maximum taken out first (as eval_metrics.hip's loss)
__device__ __forceinline__ double p1_of(double l0, double l1) {
    const double m = l0 > l1 ? l0 : l1;
    const double e0 = exp(l0 - m), e1 = exp(l1 - m);
    return e1 / (e0 + e1);
}

// One workgroup per batch.  With `has_base` row 0 of the batch is the unmodified read: its logits go to `base` (where every later
// batch of the read finds them, ordered by the stream) and to logits_out row 0, the slots are zeroed (the own-base columns of "all"
// stay 0.0: no mutant writes them) and the non-finite count starts again.  The other rows are mutants m0, m0 + 1, ...
__global__ __launch_bounds__(SCORE_THREADS) void explain_scores_kernel(const float2* __restrict__ batch, int rows, int has_base, int m0,
                                                                       const clm_explain_mutant* __restrict__ plan, int n_slots,
                                                                       float2* base, float2* __restrict__ logits_out,
                                                                       float* __restrict__ dp1, float* __restrict__ dgap,
                                                                       int* n_nonfinite) {
    __shared__ int s_bad[SCORE_WAVES];
    const int tid = (int)threadIdx.x;
    float2 b0;
    if (has_base) {
        b0 = batch[0];
        for (int i = tid; i < n_slots; i += SCORE_THREADS) { dp1[i] = 0.f; dgap[i] = 0.f; }
        if (tid == 0) { *base = b0; logits_out[0] = b0; }
        __syncthreads();                          // the zeroes are down before a mutant's slot is written
    } else {
        b0 = *base;
    }
    const double bp1 = p1_of((double)b0.x, (double)b0.y), bgap = (double)b0.y - (double)b0.x;
    const int n_mut = rows - has_base;
    int bad = 0;
    for (int r = tid; r < n_mut; r += SCORE_THREADS) {
        const float2 l = batch[r + has_base];
        const clm_explain_mutant mu = plan[m0 + r];
        logits_out[1 + m0 + r] = l;
        float d1, dg;
        if (isfinite(l.x) && isfinite(l.y)) {
            d1 = (float)(p1_of((double)l.x, (double)l.y) - bp1);     // (NaN when the base logits are not finite)
            dg = (float)(((double)l.y - (double)l.x) - bgap);
        } else {
            ++bad;
            d1 = dg = __builtin_nanf("");
        }
        if (mu.slot >= 0 && mu.slot < n_slots) { dp1[mu.slot] = d1; dgap[mu.slot] = dg; }
    }
    bad = wave_sum_i(bad);
    if ((tid & 63) == 0) s_bad[tid >> 6] = bad;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < SCORE_WAVES; ++w) bad += s_bad[w];
    *n_nonfinite = (has_base ? 0 : *n_nonfinite) + bad;
}

// ---- reduce -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool peak_before(float va, int pa, float vb, int pb) { return va > vb || (va == vb && pa < pb); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// One workgroup per read.  Dynamic LDS v[max(n_windows, n_bases)]: first the windows' max_c |d[k, c]|, then the importance.
// importance[b] = max over the windows k with k * stride <= b < k * stride + window (NaN if one of them is NaN); every thread writes
// the bases b = tid, tid + NT, ... to the caller's array and, behind the barrier that ends the windows' use of LDS, the same values
// into LDS for the selection rounds (those of attn_weights.hip: the larger value, equal values by the lower position).
template <int NT>
__global__ __launch_bounds__(NT) void explain_reduce_kernel(const float* __restrict__ d, int n_bases, int window, int stride, int n_sub,
                                                            int top_k, float* __restrict__ importance, int* __restrict__ peak_pos,
                                                            float* __restrict__ peak_val) {
    constexpr int NW = NT / 64;
    extern __shared__ float v[];
    __shared__ float red_f[2][RED_MAXW];
    __shared__ int red_i[2][RED_MAXW];
    __shared__ int red_bad[RED_MAXW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_windows = (n_bases + stride - 1) / stride;

    // 1: windows -> LDS
    for (int k = tid; k < n_windows; k += NT) {
        float m = fabsf(d[(size_t)k * n_sub]);
        for (int c = 1; c < n_sub; ++c) m = nan_max(m, fabsf(d[(size_t)k * n_sub + c]));
        v[k] = m;
    }
    __syncthreads();

    // 2: importance of this thread's bases, to the caller's array (the windows are still in LDS)
    int bad = 0;
    for (int b = tid; b < n_bases; b += NT) {
        const int k1 = b / stride;                                       // the last window that starts at or before b
        const int k0 = b < window ? 0 : (b - window) / stride + 1;       // the first window that still reaches b
        float m = v[k0];
        for (int k = k0 + 1; k <= k1; ++k) m = nan_max(m, v[k]);
        bad |= m != m;
        importance[b] = m;
    }
    bad = __any(bad);
    if (lane == 0) red_bad[wave] = bad;
    __syncthreads();                                                     // (nobody reads a window after this)
#pragma unroll
    for (int i = 0; i < NW; ++i) bad |= red_bad[i];
    const int n_peaks = bad ? 0 : min(top_k, n_bases);
    if (tid < top_k && tid >= n_peaks) {                                 // slots no peak fills (top_k <= 32 < NT)
        peak_pos[tid] = -1;
        peak_val[tid] = 0.f;
    }
    if (n_peaks == 0) return;                                            // (uniform)

    // 3: n_peaks selection rounds over LDS; a thread only ever reads the elements it wrote itself
    float bv = -1.f;
    int bp = INT_MAX;
    for (int b = tid; b < n_bases; b += NT) {
        const float x = importance[b];                                   // (this thread's own store)
        v[b] = x;
        if (x > bv) { bv = x; bp = b; }                                  // (ascending b, strict: the lower position wins a tie)
    }
    for (int k = 0; k < n_peaks; ++k) {
        float x = bv;
        int p = bp;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ox = __shfl_xor(x, o, 64);
            const int op = __shfl_xor(p, o, 64);
            if (peak_before(ox, op, x, p)) { x = ox; p = op; }
        }
        const int buf = k & 1;                                           // (two buffers: one barrier per round)
        if (lane == 0) { red_f[buf][wave] = x; red_i[buf][wave] = p; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (peak_before(red_f[buf][i], red_i[buf][i], x, p)) { x = red_f[buf][i]; p = red_i[buf][i]; }
        if (tid == 0) { peak_pos[k] = p; peak_val[k] = x; }
        if (p == bp) {                                                   // mine: strike it out (importance is >= 0), find my next best
            v[p] = -1.f;
            bv = -1.f;
            bp = INT_MAX;
            for (int b = tid; b < n_bases; b += NT)
                if (v[b] > bv) { bv = v[b]; bp = b; }
        }
    }
}

void launch_reduce(const float* d, int n_bases, int window, int stride, int n_sub, int top_k, float* importance, int* peak_pos,
                   float* peak_val, hipStream_t st) {
    // one LDS size per kernel (launch_lds): the class's capacity, not n_bases
    if (n_bases <= 2048)
        launch_lds<explain_reduce_kernel<256>>(dim3(1), dim3(256), (size_t)2048 * 4, st, d, n_bases, window, stride, n_sub, top_k,
                                               importance, peak_pos, peak_val);
    else if (n_bases <= 8448)
        launch_lds<explain_reduce_kernel<512>>(dim3(1), dim3(512), (size_t)8448 * 4, st, d, n_bases, window, stride, n_sub, top_k,
                                               importance, peak_pos, peak_val);
    else
        launch_lds<explain_reduce_kernel<1024>>(dim3(1), dim3(1024), (size_t)MAX_BASES * 4, st, d, n_bases, window, stride, n_sub, top_k,
                                                importance, peak_pos, peak_val);
}

}  // namespace explain
}  // namespace clm

using namespace clm;

struct clm_explain_handle {
    int device = 0;
    std::string err;
    DevBuf base;                                  // float2: the unmodified read's logits, written by the first batch's scores
};

namespace {

int bad_options(clm_explain_handle* h, const char* who, int n_bases, int window, int stride) {
    if (n_bases < 1 || n_bases > explain::MAX_BASES)
        return fail(h, CLM_E_INVALID, std::string(who) + ": a read has 1 ... 32768 bases, got " + std::to_string(n_bases));
    if (window < 1 || stride < 1 || stride > window)
        return fail(h, CLM_E_INVALID, std::string(who) + ": window >= 1 and 1 <= stride <= window, got window " +
                                          std::to_string(window) + ", stride " + std::to_string(stride));
    return CLM_OK;
}

}  // namespace

extern "C" {

int clm_explain_plan(const unsigned char* ids, int L, int window, int stride, int substitute, clm_explain_mutant* plan, int capacity,
                     int* n_mutants, int* n_windows) {
    clm_explain_handle* const none = nullptr;
    if (!ids || !n_mutants || !n_windows) return fail(none, CLM_E_INVALID, "clm_explain_plan: bad argument");
    if (int rc = bad_options(none, "clm_explain_plan", L - 1, window, stride)) return rc;
    if (substitute != CLM_EXPLAIN_SUB_N && substitute != CLM_EXPLAIN_SUB_ALL)
        return fail(none, CLM_E_INVALID, "clm_explain_plan: substitute is CLM_EXPLAIN_SUB_N or CLM_EXPLAIN_SUB_ALL");
    if (substitute == CLM_EXPLAIN_SUB_ALL && (window != 1 || stride != 1))
        return fail(none, CLM_E_INVALID, "clm_explain_plan: saturation mutagenesis (CLM_EXPLAIN_SUB_ALL) needs window = stride = 1");
    const int n_bases = L - 1;
    if (ids[n_bases] != explain::SEP_ID) return fail(none, CLM_E_INVALID, "clm_explain_plan: the read's last token must be [SEP] (id 1)");
    for (int t = 0; t < n_bases; ++t)
        if (ids[t] < explain::BASE_A || ids[t] > explain::BASE_N)
            return fail(none, CLM_E_INVALID, "clm_explain_plan: token " + std::to_string(t) + " is not a base (ids 7 ... 11), got " +
                                                 std::to_string((int)ids[t]));
    const int nw = (n_bases + stride - 1) / stride;
    int m = 0;
    for (int k = 0; k < nw; ++k) {
        if (substitute == CLM_EXPLAIN_SUB_N) {
            if (plan && m < capacity) plan[m] = clm_explain_mutant{k * stride, explain::BASE_N, k, 0};
            ++m;
            continue;
        }
        for (int c = 0; c < 4; ++c) {
            if (ids[k] == explain::BASE_A + c) continue;           // the read's own base: its column stays 0.0, no forward
            if (plan && m < capacity) plan[m] = clm_explain_mutant{k, explain::BASE_A + c, 4 * k + c, 0};
            ++m;
        }
    }
    *n_mutants = m;
    *n_windows = nw;
    if (plan && m > capacity)
        return fail(none, CLM_E_INVALID, "clm_explain_plan: the plan has " + std::to_string(m) + " mutants, capacity " + std::to_string(capacity));
    return CLM_OK;
}

int clm_explain_create(int device, clm_explain_handle** out) {
    if (!out) return fail<clm_explain_handle>(nullptr, CLM_E_INVALID, "clm_explain_create: bad argument");
    if (int rc = use_gfx950<clm_explain_handle>(device, "clm_explain_create")) return rc;
    clm_explain_handle* h = new clm_explain_handle();
    h->device = device;
    hipError_t e = h->base.alloc(sizeof(float2));
    if (e == hipSuccess) e = hipMemset(h->base.get(), 0, sizeof(float2));
    if (e != hipSuccess) {
        const std::string msg = std::string("clm_explain_create: ") + hipGetErrorString(e);
        delete h;
        return fail<clm_explain_handle>(nullptr, CLM_E_HIP, msg);
    }
    *out = h;
    return CLM_OK;
}

int clm_explain_rows(clm_explain_handle* h, const unsigned char* ids, int L, int window, const clm_explain_mutant* plan, int n_mutants,
                     int m0, int rows, unsigned char* out, int64_t row_stride, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!ids || !plan || !out) return fail(h, CLM_E_INVALID, "clm_explain_rows: bad argument");
    if (L < 2 || L > explain::MAX_BASES + 1 || window < 1)
        return fail(h, CLM_E_INVALID, "clm_explain_rows: L is 2 ... 32769 tokens and window >= 1");
    if (m0 < 0 || rows < 1 || rows > 65535 || (int64_t)m0 + rows > n_mutants)
        return fail(h, CLM_E_INVALID, "clm_explain_rows: mutants m0 ... m0 + rows - 1 must lie in the plan (1 ... 65535 rows), got m0 " +
                                          std::to_string(m0) + ", rows " + std::to_string(rows) + ", n_mutants " + std::to_string(n_mutants));
    if (row_stride < L || row_stride % 16 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0 || reinterpret_cast<uintptr_t>(ids) % 16 != 0)
        return fail(h, CLM_E_INVALID, "clm_explain_rows: ids and out must be 16-byte aligned and row_stride a multiple of 16 that is >= L");
    HIPCHK(h, hipSetDevice(h->device));
    const int chunks = (L + 15) / 16;
    hipLaunchKernelGGL(explain::explain_rows_kernel, dim3((chunks + explain::ROWS_THREADS - 1) / explain::ROWS_THREADS, rows),
                       dim3(explain::ROWS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ids, L, window, plan, m0, out, row_stride);
    return launched(h, "clm_explain_rows");
}

int clm_explain_scores(clm_explain_handle* h, const float* batch_logits, int rows, int has_base, const clm_explain_mutant* plan,
                       int n_mutants, int m0, int n_slots, float* logits_out, float* dp1, float* dgap, int* n_nonfinite, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!batch_logits || !plan || !logits_out || !dp1 || !dgap || !n_nonfinite || n_slots < 1)
        return fail(h, CLM_E_INVALID, "clm_explain_scores: bad argument");
    if (has_base != 0 && has_base != 1) return fail(h, CLM_E_INVALID, "clm_explain_scores: has_base is 0 or 1");
    if (has_base && m0 != 0) return fail(h, CLM_E_INVALID, "clm_explain_scores: the batch with the unmodified read starts at mutant 0");
    if (rows < 1 || m0 < 0 || (int64_t)m0 + rows - has_base > n_mutants)
        return fail(h, CLM_E_INVALID, "clm_explain_scores: the batch's mutants must lie in the plan, got m0 " + std::to_string(m0) +
                                          ", rows " + std::to_string(rows) + ", n_mutants " + std::to_string(n_mutants));
    if (reinterpret_cast<uintptr_t>(batch_logits) % 8 != 0 || reinterpret_cast<uintptr_t>(logits_out) % 8 != 0)
        return fail(h, CLM_E_INVALID, "clm_explain_scores: logits must be 8-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(explain::explain_scores_kernel, dim3(1), dim3(explain::SCORE_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float2*>(batch_logits), rows, has_base, m0, plan, n_slots, h->base.get<float2>(),
                       reinterpret_cast<float2*>(logits_out), dp1, dgap, n_nonfinite);
    return launched(h, "clm_explain_scores");
}

int clm_explain_reduce(clm_explain_handle* h, const float* d, int n_bases, int window, int stride, int n_sub, int top_k,
                       float* importance, int* peak_pos, float* peak_val, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!d || !importance || !peak_pos || !peak_val) return fail(h, CLM_E_INVALID, "clm_explain_reduce: bad argument");
    if (int rc = bad_options(h, "clm_explain_reduce", n_bases, window, stride)) return rc;
    if (n_sub != 1 && n_sub != 4) return fail(h, CLM_E_INVALID, "clm_explain_reduce: n_sub is 1 (N) or 4 (all)");
    if (top_k < 1 || top_k > ATTN_MAX_TOP_K) return fail(h, CLM_E_INVALID, "clm_explain_reduce: top_k must be 1 ... 32");
    HIPCHK(h, hipSetDevice(h->device));
    explain::launch_reduce(d, n_bases, window, stride, n_sub, top_k, importance, peak_pos, peak_val, reinterpret_cast<hipStream_t>(stream));
    return launched(h, "clm_explain_reduce");
}

const char* clm_explain_last_error(const clm_explain_handle* h) {
    return h ? h->err.c_str() : create_error<clm_explain_handle>().c_str();
}

int clm_explain_destroy(clm_explain_handle* h) { return destroy_handle(h); }

}  // extern "C"
