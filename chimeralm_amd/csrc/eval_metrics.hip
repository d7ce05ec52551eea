// eval_metrics.hip -- the test stage's metric sums on MI355X: kernel + handle + C ABI (clm_eval_*).
//
// The reference's test_step hands loss and predictions of every batch to torchmetrics on the host (a sync per batch).  Here one tiny
// kernel per batch, queued on the stream the logits were produced on, adds the batch to twelve sums in device memory; the host reads
// them once when the stage is over.  One workgroup, no atomics: lane t takes rows t, t + 256, ... in order, a wave adds its lanes in a
// fixed shuffle tree, lane 0 adds the four waves in order and then updates the sums -- the same bits on every run.
#include <cmath>
#include <string>

#include "handle_host.h"

namespace clm {
namespace eval {

constexpr int THREADS = 256, WAVES = THREADS / 64;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

enum { TP, FP, TN, FN, IGN, INV, NONF, NCOUNT };

__global__ __launch_bounds__(THREADS) void eval_update_kernel(const float2* __restrict__ logits, const int64_t* __restrict__ labels,
                                                               int B, int64_t ignore_index, clm_eval_result* __restrict__ acc) {
    __shared__ int s_cnt[WAVES][NCOUNT];
    __shared__ double s_loss[WAVES];
    int cnt[NCOUNT] = {0, 0, 0, 0, 0, 0, 0};
    double loss = 0.0;
    for (int r = (int)threadIdx.x; r < B; r += THREADS) {
        const int64_t y = labels[r];
        if (y == ignore_index) { ++cnt[IGN]; continue; }
        if (y != 0 && y != 1) { ++cnt[INV]; continue; }
        const float2 l = logits[r];
        if (!(isfinite(l.x) && isfinite(l.y))) { ++cnt[NONF]; continue; }
        const double l0 = (double)l.x, l1 = (double)l.y, m = l0 > l1 ? l0 : l1;
        const double lse = log(exp(l0 - m) + exp(l1 - m));          // log-sum-exp with the maximum taken out
        loss += lse - ((y ? l1 : l0) - m);
        const bool pred = l.y > l.x;                                // a tie is class 0, as torch.argmax
        ++cnt[pred ? (y ? TP : FP) : (y ? FN : TN)];
    }
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NCOUNT; ++i) cnt[i] = wave_sum(cnt[i]);
    loss = wave_sum(loss);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NCOUNT; ++i) s_cnt[wave][i] = cnt[i];
        s_loss[wave] = loss;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < WAVES; ++w) {
#pragma unroll
        for (int i = 0; i < NCOUNT; ++i) cnt[i] += s_cnt[w][i];
        loss += s_loss[w];
    }
    const int valid = cnt[TP] + cnt[FP] + cnt[TN] + cnt[FN];
    acc->n_invalid_labels += cnt[INV];
    acc->n_nonfinite += cnt[NONF];
    if (valid == 0) {
        acc->n_empty_batches += 1;
        return;
    }
    acc->tp += cnt[TP];
    acc->fp += cnt[FP];
    acc->tn += cnt[TN];
    acc->fn += cnt[FN];
    acc->n_valid += valid;
    acc->n_ignored += cnt[IGN];
    acc->n_batches += 1;
    acc->sum_batch_mean_loss += loss / (double)valid;
    acc->sum_loss += loss;
}

void add(clm_eval_result& a, const clm_eval_result& b) {
    a.tp += b.tp; a.fp += b.fp; a.tn += b.tn; a.fn += b.fn;
    a.n_valid += b.n_valid; a.n_ignored += b.n_ignored; a.n_batches += b.n_batches; a.n_empty_batches += b.n_empty_batches;
    a.n_invalid_labels += b.n_invalid_labels; a.n_nonfinite += b.n_nonfinite;
    a.sum_batch_mean_loss += b.sum_batch_mean_loss; a.sum_loss += b.sum_loss;
}

}  // namespace eval
}  // namespace clm

using namespace clm;

struct clm_eval_handle {
    int device = 0;
    int64_t ignore_index = -100;
    std::string err;
    DevBuf acc;                                   // one clm_eval_result, updated by the kernel
    clm_eval_result* staging = nullptr;           // page-locked: clm_eval_read's copy target
    clm_eval_result merged{};                     // other ranks' sums (clm_eval_merge)
};

extern "C" {

int clm_eval_create(int device, int n_classes, int64_t ignore_index, clm_eval_handle** out) {
    if (!out) return fail<clm_eval_handle>(nullptr, CLM_E_INVALID, "clm_eval_create: bad argument");
    if (n_classes != 2)
        return fail<clm_eval_handle>(nullptr, CLM_E_INVALID, "clm_eval_create: binary metrics only, n_classes must be 2, got " +
                                                                 std::to_string(n_classes));
    if (ignore_index == 0 || ignore_index == 1)
        return fail<clm_eval_handle>(nullptr, CLM_E_INVALID, "clm_eval_create: ignore_index must not be one of the classes 0 / 1");
    if (device < 0) {                                          // host-only: a place to total the ranks' results
        clm_eval_handle* h = new clm_eval_handle();
        h->device = -1;
        h->ignore_index = ignore_index;
        *out = h;
        return CLM_OK;
    }
    if (int rc = use_gfx950<clm_eval_handle>(device, "clm_eval_create")) return rc;
    clm_eval_handle* h = new clm_eval_handle();
    h->device = device;
    h->ignore_index = ignore_index;
    hipError_t e = h->acc.alloc(sizeof(clm_eval_result));
    if (e == hipSuccess) e = hipMemset(h->acc.get(), 0, sizeof(clm_eval_result));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->staging), sizeof(clm_eval_result), hipHostMallocDefault);
    if (e != hipSuccess) {
        const std::string msg = std::string("clm_eval_create: ") + hipGetErrorString(e);
        delete h;
        return fail<clm_eval_handle>(nullptr, CLM_E_HIP, msg);
    }
    *out = h;
    return CLM_OK;
}

int clm_eval_update(clm_eval_handle* h, const float* logits, const int64_t* labels, int B, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (h->device < 0) return fail(h, CLM_E_STATE, "clm_eval_update: a host-only handle (device -1) only merges");
    if (!logits || !labels || B < 1) return fail(h, CLM_E_INVALID, "clm_eval_update: bad argument");
    if (reinterpret_cast<uintptr_t>(logits) % 8 != 0) return fail(h, CLM_E_INVALID, "clm_eval_update: logits must be 8-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(eval::eval_update_kernel, dim3(1), dim3(eval::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float2*>(logits), labels, B, h->ignore_index, h->acc.get<clm_eval_result>());
    return launched(h, "clm_eval_update");
}

int clm_eval_read(clm_eval_handle* h, clm_eval_result* out, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!out) return fail(h, CLM_E_INVALID, "clm_eval_read: bad argument");
    if (h->device < 0) {
        *out = h->merged;
        return CLM_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipMemcpyAsync(h->staging, h->acc.get(), sizeof(clm_eval_result), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    *out = *h->staging;
    eval::add(*out, h->merged);
    return CLM_OK;
}

int clm_eval_merge(clm_eval_handle* h, const clm_eval_result* other) {
    if (!h) return CLM_E_INVALID;
    if (!other) return fail(h, CLM_E_INVALID, "clm_eval_merge: bad argument");
    eval::add(h->merged, *other);
    return CLM_OK;
}

int clm_eval_reset(clm_eval_handle* h, void* stream) {
    if (!h) return CLM_E_INVALID;
    h->merged = clm_eval_result{};
    if (h->device < 0) return CLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->acc.get(), 0, sizeof(clm_eval_result), reinterpret_cast<hipStream_t>(stream)));
    return CLM_OK;
}

const char* clm_eval_last_error(const clm_eval_handle* h) { return h ? h->err.c_str() : create_error<clm_eval_handle>().c_str(); }

int clm_eval_destroy(clm_eval_handle* h) {
    return destroy_handle(h, [h] {
        if (h->staging) (void)hipHostFree(h->staging);
    });
}

}  // extern "C"
