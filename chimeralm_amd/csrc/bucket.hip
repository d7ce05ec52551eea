// bucket.hip -- length-bucketed predict on MI355X: the kernel that moves the reads of an incoming batch into the rows of their
// classes' slabs, a handle and the C ABI (clm_bucket_create / _scatter / _last_error / _destroy).  The host plan is
// csrc/bucket_plan.cpp; the definitions are in include/chimeralm_hip.h.
//
// The reference pads a batch to its longest read (/root/reference/chimeralm/data/tokenizer.py:152-159).  Here a read's row is
// [PAD] x (Lc - n) and its n tokens, Lc a function of n alone; bucket_scatter_kernel writes such rows at per-row offsets of a pool,
// from the left-padded uint8 batch that is already on the device.  It is queued on the caller's stream, in front of the forward
// that reads the rows; no atomics, every destination byte is written once by one thread: bitwise the same from run to run.
#include <cstring>
#include <string>

#include "handle_host.h"

namespace clm {
namespace bucket {

constexpr int THREADS = 256;                   // bucket_scatter_kernel: one 16-byte chunk of one destination row per thread
constexpr int SLOTS = 8;                       // a handle's span buffer is a ring of this many slots, used in turn ...
constexpr int SLOT_SPANS = 4096;               // ... of this many spans each: a longer group goes out as several launches

// Destination row blockIdx.y is span spans[blockIdx.y]: [PAD] x (dst_width - n_copy), the n_copy bytes of source row src_row from
// column src_col, zeroes up to the next multiple of 16.  A thread owns 16 consecutive destination bytes and stores them once.
// Their source starts at an arbitrary byte: the two aligned 16-byte blocks around it are loaded and funnelled per dword
// (v_alignbyte_b32), as longread_rows_kernel does for one output buffer.  An aligned block is loaded only if it lies inside
// [0, total): ids is 16-byte aligned and total = B * row_stride a multiple of 16, so no load leaves the batch whatever the spans
// hold; a store is issued only if its 16 bytes lie inside [0, pool_bytes).
__global__ __launch_bounds__(THREADS) void bucket_scatter_kernel(const unsigned char* __restrict__ ids, int64_t row_stride, int64_t total,
                                                                 const clm_bucket_span* __restrict__ spans,
                                                                 unsigned char* __restrict__ pool, int64_t pool_bytes) {
    const clm_bucket_span sp = spans[blockIdx.y];
    const int j0 = (int)(blockIdx.x * THREADS + threadIdx.x) * 16;
    const int width = sp.dst_width;
    if (j0 >= width) return;
    const int pad = width - sp.n_copy;                                       // columns [pad, width) are copied
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (j0 + 16 > pad) {                                                     // (the copy meets this chunk)
        const int64_t g = (int64_t)sp.src_row * row_stride + sp.src_col + (j0 - pad);   // source of column j0 (may lie before 0)
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
    if (j0 < pad || j0 + 16 > width) {                                       // pads or the row's end in this chunk
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned keep = 0u, fill = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = j0 + 4 * i + b;
                if (j >= pad && j < width) keep |= 0xFFu << (8 * b);
                else fill |= (j < pad ? (unsigned)PAD_ID : 0u) << (8 * b);
            }
            w[i] = (w[i] & keep) | fill;
        }
    }
    const int64_t o = sp.dst_offset + j0;
    if (o >= 0 && o + 16 <= pool_bytes) *reinterpret_cast<uint4*>(pool + o) = make_uint4(w[0], w[1], w[2], w[3]);
}

// The spans of a launch go to the device through slot `next` of a ring in page-locked host memory and its device copy, both
// allocated once by clm_bucket_create; a slot is reused after the event behind the launch that read it.
struct Ring {
    void* host = nullptr;                      // [SLOTS][SLOT_SPANS] clm_bucket_span, page-locked
    DevBuf dev;                                // the same on the device
    hipEvent_t done[SLOTS] = {};
    bool used[SLOTS] = {};
    int next = 0;
};

}  // namespace bucket
}  // namespace clm

using namespace clm;

struct clm_bucket_handle {
    int device = 0;
    std::string err;
    bucket::Ring ring;
};

namespace {

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int clm_bucket_create(int device, clm_bucket_handle** out) {
    if (!out) return fail<clm_bucket_handle>(nullptr, CLM_E_INVALID, "clm_bucket_create: bad argument");
    if (int rc = use_gfx950<clm_bucket_handle>(device, "clm_bucket_create")) return rc;
    clm_bucket_handle* h = new clm_bucket_handle();
    h->device = device;
    const size_t bytes = (size_t)bucket::SLOTS * bucket::SLOT_SPANS * sizeof(clm_bucket_span);
    hipError_t e = hipHostMalloc(&h->ring.host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = h->ring.dev.alloc(bytes);
    for (int i = 0; i < bucket::SLOTS && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->ring.done[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        fail<clm_bucket_handle>(nullptr, CLM_E_HIP, std::string("clm_bucket_create: ") + hipGetErrorString(e));
        clm_bucket_destroy(h);
        return CLM_E_HIP;
    }
    *out = h;
    return CLM_OK;
}

int clm_bucket_scatter(clm_bucket_handle* h, const unsigned char* ids, int64_t row_stride, int B, int L, const clm_bucket_span* spans,
                       int n_spans, int s0, int rows, unsigned char* pool, int64_t pool_bytes, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!ids || !spans || !pool || B < 1 || L < 1 || pool_bytes < 16) return fail(h, CLM_E_INVALID, "clm_bucket_scatter: bad argument");
    if (!aligned16(ids) || row_stride < L || row_stride % 16 != 0)
        return fail(h, CLM_E_INVALID, "clm_bucket_scatter: ids must be 16-byte aligned and row_stride a multiple of 16 that is >= L");
    if (!aligned16(pool)) return fail(h, CLM_E_INVALID, "clm_bucket_scatter: the pool must be 16-byte aligned");
    if (s0 < 0 || rows < 1 || rows > 65535 || (int64_t)s0 + rows > n_spans)
        return fail(h, CLM_E_INVALID, "clm_bucket_scatter: spans s0 ... s0 + rows - 1 must lie in the plan (1 ... 65535 rows), got s0 " +
                                          std::to_string(s0) + ", rows " + std::to_string(rows) + ", n_spans " + std::to_string(n_spans));
    for (int i = s0; i < s0 + rows; ++i) {
        const clm_bucket_span& sp = spans[i];
        const int64_t w16 = ((int64_t)sp.dst_width + 15) / 16 * 16;
        if (sp.src_row < 0 || sp.src_row >= B || sp.src_col < 0 || sp.n_copy < 1 || (int64_t)sp.src_col + sp.n_copy > L ||
            sp.dst_width < sp.n_copy || sp.dst_width > CLM_BUCKET_MAX_TOKENS)
            return fail(h, CLM_E_INVALID, "clm_bucket_scatter: span " + std::to_string(i) + " leaves its source row or its own width, or "
                                          "is wider than 32769");
        if (sp.dst_offset < 0 || sp.dst_offset % 16 != 0 || sp.dst_offset > pool_bytes - w16)
            return fail(h, CLM_E_INVALID, "clm_bucket_scatter: span " + std::to_string(i) + " leaves the pool or is not at a 16-byte "
                                          "offset (offset " + std::to_string(sp.dst_offset) + ", width " + std::to_string(sp.dst_width) +
                                          ", pool " + std::to_string(pool_bytes) + " bytes)");
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bucket::Ring& ring = h->ring;
    for (int r0 = 0; r0 < rows; r0 += bucket::SLOT_SPANS) {
        const int n = rows - r0 < bucket::SLOT_SPANS ? rows - r0 : bucket::SLOT_SPANS;
        const int slot = ring.next;
        if (ring.used[slot]) HIPCHK(h, hipEventSynchronize(ring.done[slot]));    // the launch eight launches back has read this slot
        ring.used[slot] = false;
        clm_bucket_span* host = static_cast<clm_bucket_span*>(ring.host) + (size_t)slot * bucket::SLOT_SPANS;
        clm_bucket_span* dev = ring.dev.get<clm_bucket_span>() + (size_t)slot * bucket::SLOT_SPANS;
        std::memcpy(host, spans + s0 + r0, (size_t)n * sizeof(clm_bucket_span));
        int max_width = 0;
        for (int i = 0; i < n; ++i) max_width = host[i].dst_width > max_width ? host[i].dst_width : max_width;
        HIPCHK(h, hipMemcpyAsync(dev, host, (size_t)n * sizeof(clm_bucket_span), hipMemcpyHostToDevice, st));
        const int chunks = (max_width + 15) / 16;                                // (<= 2049: dst_width <= 32769)
        hipLaunchKernelGGL(bucket::bucket_scatter_kernel, dim3((chunks + bucket::THREADS - 1) / bucket::THREADS, n), dim3(bucket::THREADS),
                           0, st, ids, row_stride, (int64_t)B * row_stride, dev, pool, pool_bytes);
        if (int rc = launched(h, "clm_bucket_scatter")) return rc;
        HIPCHK(h, hipEventRecord(ring.done[slot], st));
        ring.used[slot] = true;
        ring.next = (slot + 1) % bucket::SLOTS;
    }
    return CLM_OK;
}

const char* clm_bucket_last_error(const clm_bucket_handle* h) { return h ? h->err.c_str() : create_error<clm_bucket_handle>().c_str(); }

int clm_bucket_destroy(clm_bucket_handle* h) {
    return destroy_handle(h, [h] {
        if (h->ring.host) (void)hipHostFree(h->ring.host);
        for (hipEvent_t e : h->ring.done)
            if (e) (void)hipEventDestroy(e);
    });
}

}  // extern "C"
