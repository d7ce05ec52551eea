// longread.hip -- reads longer than the model's context on MI355X: two kernels around the nets' own forwards, a handle and the C ABI
// (clm_longread_*).  The host plan is csrc/longread_plan.cpp.
//
// The reference truncates a read to the tokenizer's 32,768 bases (/root/reference/chimeralm/data/bam.py:166-170); what lies
// behind them reaches no net.  Here the untruncated, left-padded uint8 batch is on the device; longread_rows_kernel writes the rows
// the forwards take -- the head batch (byte for byte what the truncating path delivers) and the extra windows of the long reads,
// both as spans of the plan -- the forward is the net's own, and longread_reduce_kernel picks per read the window with the largest
// logit1 - logit0.  Everything is queued on the caller's stream; no atomics, one thread per read walks its windows in order:
// bitwise the same from run to run.
#include <string>

#include "handle_host.h"
#include "longread_plan.h"

namespace clm {
namespace longread {

constexpr int ROWS_THREADS = 256;              // longread_rows_kernel: one 16-byte chunk of one output row per thread
constexpr int REDUCE_THREADS = 256;            // longread_reduce_kernel: one read per thread

// ---- rows ---------------------------------------------------------------------------------------------------------------------
// Output row r is span s0 + r: [PAD] x (width - n_copy - sep), the n_copy bytes of source row `read` from column src_col, [SEP] if
// bit 0 of flags is set, zeroes up to the next multiple of 16.  A thread owns 16 consecutive output bytes and stores them once.
// Their source starts at an arbitrary byte: the two aligned 16-byte blocks around it are loaded and funnelled per dword
// (v_alignbyte_b32).  An aligned block is loaded only if it lies inside [0, total): ids is 16-byte aligned and total = B *
// row_stride a multiple of 16, so no load leaves the allocation whatever the spans hold; bytes of a block that was not loaded are
// never selected by a span that lies inside its row.
__global__ __launch_bounds__(ROWS_THREADS) void longread_rows_kernel(const unsigned char* __restrict__ ids, int64_t row_stride, int64_t total,
                                                                     const clm_longread_span* __restrict__ spans, int s0,
                                                                     unsigned char* __restrict__ out, int64_t out_stride, int width) {
    const int chunk = (int)(blockIdx.x * ROWS_THREADS + threadIdx.x);
    const int j0 = chunk * 16;
    if (j0 >= width) return;
    const clm_longread_span sp = spans[s0 + (int)blockIdx.y];
    const int sep = sp.flags & CLM_LONGREAD_SEP;
    const int pad = width - sp.n_copy - sep, end = pad + sp.n_copy;          // columns [pad, end) are copied
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (j0 + 16 > pad && j0 < end) {                                         // (the copy meets this chunk)
        const int64_t g = (int64_t)sp.read * row_stride + sp.src_col + (j0 - pad);   // source of output column j0 (may lie before 0)
        const int64_t a = g & ~(int64_t)15;                                  // (floor, also below 0)
        const int sh = (int)(g - a);
        uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
        if (a >= 0 && a < total) lo = *reinterpret_cast<const uint4*>(ids + a);
        if (sh != 0 && a + 16 >= 0 && a + 16 < total) hi = *reinterpret_cast<const uint4*>(ids + a + 16);
        const unsigned d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const int q = sh >> 2;
        const unsigned r = (unsigned)(sh & 3);
        unsigned e[5];                                                       // dwords q ... q + 4 (constant indices: registers, no scratch)
#pragma unroll
        for (int i = 0; i < 5; ++i) e[i] = q == 0 ? d[i] : q == 1 ? d[i + 1] : q == 2 ? d[i + 2] : d[i + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = __builtin_amdgcn_alignbyte(e[i + 1], e[i], r);
    }
    if (j0 < pad || j0 + 16 > end) {                                         // pads, [SEP] or the row's end in this chunk
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned keep = 0u, fill = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = j0 + 4 * i + b;
                if (j >= pad && j < end) keep |= 0xFFu << (8 * b);
                else fill |= (j < pad ? (unsigned)PAD_ID : j < width ? (unsigned)SEP_ID : 0u) << (8 * b);
            }
            w[i] = (w[i] & keep) | fill;
        }
    }
    *reinterpret_cast<uint4*>(out + (size_t)blockIdx.y * out_stride + j0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- reduce -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite2(float2 l) { return isfinite(l.x) && isfinite(l.y); }

// One thread per read.  Window 0 of read r is logits row r, its extra windows are rows B + first[r] ... B + first[r + 1] - 1.
// gap = (double)logit1 - (double)logit0 of every window is written as fp32; the chosen window has the largest gap (equal gaps: the
// lowest index), or is the first window with a non-finite logit if there is one.  Its two floats are copied bit for bit.
__global__ __launch_bounds__(REDUCE_THREADS) void longread_reduce_kernel(const uint2* __restrict__ logits, const int* __restrict__ first,
                                                                         int B, uint2* __restrict__ logits_out, int* __restrict__ chosen,
                                                                         float* __restrict__ gap, int* __restrict__ nonfinite) {
    const int r = (int)(blockIdx.x * REDUCE_THREADS + threadIdx.x);
    if (r >= B) return;
    const int e0 = first[r], n_extra = first[r + 1] - e0;
    uint2 best = logits[r];
    int best_k = 0, bad = 0, bad_k = -1;
    uint2 bad_bits = best;
    double best_gap = 0.0;
    bool have = false;
    for (int k = 0; k <= n_extra; ++k) {
        const int row = k == 0 ? r : B + e0 + k - 1;
        const uint2 bits = logits[row];
        const float2 l = make_float2(__uint_as_float(bits.x), __uint_as_float(bits.y));
        const double g = (double)l.y - (double)l.x;
        gap[row] = (float)g;
        if (!finite2(l)) {
            if (bad_k < 0) { bad_k = k; bad_bits = bits; }
            ++bad;
        } else if (!have || g > best_gap) {
            have = true;
            best_gap = g;
            best_k = k;
            best = bits;
        }
    }
    logits_out[r] = bad ? bad_bits : best;
    chosen[r] = bad ? bad_k : best_k;
    nonfinite[r] = bad;
}

}  // namespace longread
}  // namespace clm

using namespace clm;

struct clm_longread_handle {
    int device = 0;
    std::string err;
};

namespace {

// errors of a call without a handle share the text of the host plan's (clm_longread_last_error(NULL))
int fail_lr(clm_longread_handle* h, int code, const std::string& msg) {
    (h ? h->err : longread::host_error()) = msg;
    return code;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int clm_longread_create(int device, clm_longread_handle** out) {
    if (!out) return fail_lr(nullptr, CLM_E_INVALID, "clm_longread_create: bad argument");
    if (int rc = use_gfx950<clm_longread_handle>(device, "clm_longread_create")) {
        longread::host_error() = create_error<clm_longread_handle>();
        return rc;
    }
    clm_longread_handle* h = new clm_longread_handle();
    h->device = device;
    *out = h;
    return CLM_OK;
}

int clm_longread_rows(clm_longread_handle* h, const unsigned char* ids, int64_t row_stride, int B, int L, const clm_longread_span* spans,
                      int n_spans, int s0, int rows, unsigned char* out, int64_t out_stride, int width, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!ids || !spans || !out || B < 1 || L < 1 || width < 1) return fail_lr(h, CLM_E_INVALID, "clm_longread_rows: bad argument");
    if (!aligned16(ids) || row_stride < L || row_stride % 16 != 0)
        return fail_lr(h, CLM_E_INVALID, "clm_longread_rows: ids must be 16-byte aligned and row_stride a multiple of 16 that is >= L");
    if (!aligned16(out) || out_stride % 16 != 0 || out_stride < ((int64_t)width + 15) / 16 * 16)
        return fail_lr(h, CLM_E_INVALID, "clm_longread_rows: out must be 16-byte aligned and out_stride a multiple of 16 that holds "
                                         "width rounded up to 16");
    if (s0 < 0 || rows < 1 || rows > 65535 || (int64_t)s0 + rows > n_spans)
        return fail_lr(h, CLM_E_INVALID, "clm_longread_rows: spans s0 ... s0 + rows - 1 must lie in the plan (1 ... 65535 rows), got s0 " +
                                             std::to_string(s0) + ", rows " + std::to_string(rows) + ", n_spans " + std::to_string(n_spans));
    HIPCHK(h, hipSetDevice(h->device));
    const int chunks = (width + 15) / 16;
    hipLaunchKernelGGL(longread::longread_rows_kernel, dim3((chunks + longread::ROWS_THREADS - 1) / longread::ROWS_THREADS, rows),
                       dim3(longread::ROWS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ids, row_stride, (int64_t)B * row_stride, spans,
                       s0, out, out_stride, width);
    return launched(h, "clm_longread_rows");
}

int clm_longread_reduce(clm_longread_handle* h, const float* logits, const int32_t* first, int B, float* logits_out, int32_t* chosen,
                        float* gap, int32_t* nonfinite, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!logits || !first || !logits_out || !chosen || !gap || !nonfinite || B < 1)
        return fail_lr(h, CLM_E_INVALID, "clm_longread_reduce: bad argument");
    if (reinterpret_cast<uintptr_t>(logits) % 8 != 0 || reinterpret_cast<uintptr_t>(logits_out) % 8 != 0)
        return fail_lr(h, CLM_E_INVALID, "clm_longread_reduce: logits must be 8-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(longread::longread_reduce_kernel, dim3((B + longread::REDUCE_THREADS - 1) / longread::REDUCE_THREADS),
                       dim3(longread::REDUCE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint2*>(logits), first, B,
                       reinterpret_cast<uint2*>(logits_out), chosen, gap, nonfinite);
    return launched(h, "clm_longread_reduce");
}

const char* clm_longread_last_error(const clm_longread_handle* h) { return h ? h->err.c_str() : longread::host_error().c_str(); }

int clm_longread_destroy(clm_longread_handle* h) { return destroy_handle(h); }

}  // extern "C"
