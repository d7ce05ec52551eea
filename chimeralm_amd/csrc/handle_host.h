// handle_host.h -- the host side of the engine handles: what every C handle (clm_api.hip, tf_model.hip, cnn.hip, mamba.hip, the train
// handles, explain / bucket / longread / eval) does around its launches.  Device memory and the error path, the weight tables, and one
// copy each of: growing a workspace, checking the ids and trajectory arguments, reading the launch error, the end of a debug fetch,
// destroying a handle, the run mode's scope, the self-check's comparison and the stage profile.  Kernel-only files do not include it.
#pragma once
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "clm_common.h"

namespace clm {

// ---- host side of the engine handles (clm_api.hip, tf_model.hip, cnn.hip) ------------------------------------------------------
// One device allocation and its size, freed by its owner.  Nothing here synchronises: whoever replaces memory that queued kernels
// may still read synchronises first.
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t bytes) {              // what it held is freed first
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e == hipSuccess) n_ = bytes;
        else p_ = nullptr;
        return e;
    }
    hipError_t reserve(size_t bytes) { return bytes > n_ ? alloc(bytes) : hipSuccess; }   // grows, never shrinks
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    size_t bytes() const { return n_; }
    template <class T = void>
    T* get() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    void* p_ = nullptr;
    size_t n_ = 0;
};

// The last error of a handle is its `err`; before a handle exists (its *_create), one string per handle type.
template <class H>
std::string& create_error() {
    static std::string s;
    return s;
}
template <class H>
int fail(H* h, int code, const std::string& msg) {
    (h ? h->err : create_error<H>()) = msg;
    return code;
}
#define HIPCHK(h, expr)                                                                                   \
    do {                                                                                                  \
        const hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return clm::fail(h, CLM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// *_create: `device` exists, is made current and is a gfx950
template <class H>
int use_gfx950(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail<H>(nullptr, CLM_E_HIP, std::string(who) + ": no such HIP device " + std::to_string(device));
    if (hipSetDevice(device) != hipSuccess) return fail<H>(nullptr, CLM_E_HIP, std::string(who) + ": hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail<H>(nullptr, CLM_E_HIP, std::string(who) + ": hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail<H>(nullptr, CLM_E_UNSUPPORTED, std::string(who) + ": this engine is built for gfx950 (MI355X) only, found " + prop.gcnArchName);
    return CLM_OK;
}

// ---- expected weights of the transformer, CNN and Mamba engines: a handle's `expected` table, built ONCE by its *_create --------
// canonical key -> shape and where *_finalize puts the device pointer (a field of the handle; null: read by finalize alone).
// Sorted by key: the first missing weight finalize names is the first in key order.
struct WeightSpec {
    std::vector<int64_t> shape;
    const float** dst;
};
using WeightTable = std::map<std::string, WeightSpec>;

inline std::string canonical_weight_key(const char* key) {       // a Lightning checkpoint's "net." prefix is optional
    const std::string k(key);
    return k.rfind("net.", 0) == 0 ? k.substr(4) : k;
}
// `n` fp32 values as tensor `k` of the handle's `w`: a device copy, replacing the one loaded before
template <class H>
int store_f32(H* h, const std::string& k, const void* data, size_t n) {
    HIPCHK(h, hipSetDevice(h->device));
    h->w.erase(k);
    DevBuf d;
    HIPCHK(h, d.alloc(n * 4));
    HIPCHK(h, hipMemcpy(d.get(), data, n * 4, hipMemcpyDefault));
    h->w.emplace(k, std::move(d));
    h->finalized = false;
    return CLM_OK;
}
// *_load_weight: an fp32 tensor `k` of the handle's table, checked against it
template <class H>
int load_f32(H* h, const char* who, const std::string& k, const void* data, const int64_t* shape, int ndim) {
    const auto it = h->expected.find(k);
    if (it == h->expected.end()) return fail(h, CLM_E_INVALID, std::string(who) + ": unknown key " + k);
    if (it->second.shape != std::vector<int64_t>(shape, shape + ndim)) return fail(h, CLM_E_INVALID, std::string(who) + ": wrong shape for " + k);
    size_t n = 1;
    for (int64_t s : it->second.shape) n *= (size_t)s;
    return store_f32(h, k, data, n);
}
// *_finalize: every tensor of the table is loaded (else CLM_E_MISSING) and its device pointer stands where the forward reads it
template <class H>
int resolve_weights(H* h, const char* who) {
    for (const auto& kv : h->expected) {
        const auto it = h->w.find(kv.first);
        if (it == h->w.end()) return fail(h, CLM_E_MISSING, std::string(who) + ": missing weight " + kv.first);
        if (kv.second.dst) *kv.second.dst = it->second.template get<float>();
    }
    return CLM_OK;
}
// *_finalize: loaded tensor `k` back on the host (what finalize computes in fp64 or repacks there), and a product of it up again
template <class H>
int host_f32(H* h, const char* who, const std::string& k, std::vector<float>& out) {
    const auto it = h->w.find(k);
    if (it == h->w.end()) return fail(h, CLM_E_MISSING, std::string(who) + ": missing weight " + k);
    out.resize(it->second.bytes() / 4);
    HIPCHK(h, hipMemcpy(out.data(), it->second.get(), it->second.bytes(), hipMemcpyDeviceToHost));
    return CLM_OK;
}
template <class H>
int upload_f32(H* h, DevBuf& d, const std::vector<float>& src) {
    HIPCHK(h, d.alloc(src.size() * 4));
    HIPCHK(h, hipMemcpy(d.get(), src.data(), src.size() * 4, hipMemcpyHostToDevice));
    return CLM_OK;
}
// W [rows][cols] -> [cols][rows] on the host (a layer whose threads each own an output reads its weights coalesced)
inline std::vector<float> transposed(const std::vector<float>& W, int rows, int cols) {
    std::vector<float> t((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = W[(size_t)r * cols + c];
    return t;
}
// A convolution's taps, split as [taps][co][ci] fp32 on the device, each packed by pack(tap, dst) into tap_bytes of `out`.
// Synchronises before it returns: the caller reuses or frees `split` next.
template <class H, class Pack>
int pack_taps(H* h, const float* split, int taps, size_t tap_bytes, DevBuf& out, Pack pack) {
    HIPCHK(h, out.alloc(taps * tap_bytes));
    for (int dk = 0; dk < taps; ++dk) pack(split + (size_t)dk * D * D, out.get<char>() + dk * tap_bytes);
    HIPCHK(h, hipDeviceSynchronize());
    return CLM_OK;
}

// fp16x3 packs a weight x 2^10 as fp16 hi + lo (tail32.hip pack_x3_kernel): from |w| = 65504 / 2^10 ~ 63.97 the hi half saturates
// and the packing no longer holds the weight, so a handle whose x3-packed weights reach this runs its exact-fp32 kernels instead.
constexpr float X3_WEIGHT_LIMIT = 64.f;
// Largest |w| of `n` fp32 values in device memory (read back to the host; NaN as soon as one of them is NaN).
inline hipError_t device_max_abs(const float* d, size_t n, float& out) {
    std::vector<float> host(n);
    const hipError_t e = hipMemcpy(host.data(), d, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    out = 0.f;
    for (const float x : host) {
        if (x != x) { out = x; break; }
        out = __builtin_fabsf(x) > out ? __builtin_fabsf(x) : out;
    }
    return hipSuccess;
}

// ---- one copy of what every handle's calls do around their launches ----------------------------------------------------------------
// What a growing workspace waits for before it replaces memory: everything queued on the device, or the work of one stream.
struct Sync {
    bool device;
    hipStream_t st;
    static Sync Device() { return {true, nullptr}; }
    static Sync Stream(hipStream_t s) { return {false, s}; }
    hipError_t wait() const { return device ? hipDeviceSynchronize() : hipStreamSynchronize(st); }
};
struct Want {
    DevBuf* buf;
    size_t bytes;
};
// The workspace of a call: no buffer short -- nothing happens; otherwise ONE wait, then each short buffer grows on its own
template <class H>
int grow(H* h, Sync sync, std::initializer_list<Want> want) {
    bool any = false;
    for (const Want& w : want) any |= w.bytes > w.buf->bytes();
    if (!any) return CLM_OK;
    HIPCHK(h, sync.wait());
    for (const Want& w : want) HIPCHK(h, w.buf->reserve(w.bytes));
    return CLM_OK;
}

// The ids argument of `who`: B reads of L >= min_L tokens, rows `row_stride` elements apart; out: the pointer that call writes its
// result through
template <class H>
int check_ids_arg(H* h, const char* who, const void* ids, const void* out, int ids_dtype, int64_t row_stride, int B, int L, int min_L = 1) {
    const std::string w(who);
    if (!ids || !out || B < 1 || L < 1 || row_stride < L) return fail(h, CLM_E_INVALID, w + ": bad argument");
    if (L < min_L)
        return fail(h, CLM_E_INVALID, w + ": bad argument (L >= " + std::to_string(min_L) + "): this net needs reads of at least " +
                                          std::to_string(min_L) + " tokens, got L = " + std::to_string(L));
    if (ids_dtype != CLM_DT_I64 && ids_dtype != CLM_DT_I32 && ids_dtype != CLM_DT_U8)
        return fail(h, CLM_E_INVALID, w + ": ids dtype must be i64, i32 or u8");
    return CLM_OK;
}

// The trajectory request of `who` for reads of L tokens (null: none, nothing to check): what holds for every net
template <class H>
int check_traj_request(H* h, const char* who, const clm_traj_out* t, int L) {
    if (!t) return CLM_OK;
    const std::string w(who);
    if (t->struct_size != (int32_t)sizeof(clm_traj_out)) return fail(h, CLM_E_INVALID, w + ": clm_traj_out size mismatch");
    if (t->stride < 128 || t->stride > 4096 || t->stride % 128)
        return fail(h, CLM_E_INVALID, w + ": the trajectory's stride must be a multiple of 128 in 128 ... 4096");
    if (!t->logits) return fail(h, CLM_E_INVALID, w + ": the trajectory request has no logits buffer");
    const int K = (L + t->stride - 1) / t->stride;
    if (t->point_stride < K)
        return fail(h, CLM_E_INVALID, w + ": point_stride is shorter than the " + std::to_string(K) + " points of a read");
    return CLM_OK;
}

// Behind the launches of `who`: the launch error, read ONCE (reading clears it) and named in the message
template <class H>
int launched(H* h, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CLM_OK : fail(h, CLM_E_HIP, std::string(who) + ": launch failed: " + hipGetErrorString(e));
}

// The end of every *_debug_fetch: the first `bytes` of the `have` bytes the last forward left of `name` at `src`
template <class H>
int fetch_bytes(H* h, const char* who, const std::string& name, const void* src, size_t have, void* host_out, size_t bytes) {
    if (bytes > have)
        return fail(h, CLM_E_INVALID, std::string(who) + ": more bytes requested than the last forward produced (" + name + " holds " +
                                          std::to_string(have) + " bytes)");
    HIPCHK(h, hipMemcpy(host_out, src, bytes, hipMemcpyDeviceToHost));
    return CLM_OK;
}

// *_destroy: the device idle, then the handle (its DevBufs and its profile's events free themselves).  release_rest: what the
// handle owns beyond those, released in between -- behind the queued work that may still use it (a host-only handle has device < 0)
template <class H, class F>
int destroy_handle(H* h, F release_rest) {
    if (!h) return CLM_OK;
    if (h->device >= 0) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
    }
    release_rest();
    delete h;
    return CLM_OK;
}
template <class H>
int destroy_handle(H* h) {
    return destroy_handle(h, [] {});
}

// "Run forwards in this mode for a while": h->run is put back as it stood on every way out of the scope.  Profiling is off
// inside: what a handle runs for itself is not part of anybody's timed region.
template <class H>
struct RunScope {
    H* const h;
    const decltype(H::run) saved;
    explicit RunScope(H* h_) : h(h_), saved(h_->run) { h->run.prof = false; }
    ~RunScope() { h->run = saved; }
};

// The end of a self-check: pair [2][B][NCLS] fp32 logits of its two forwards on the device -> their largest deviation and the
// number of reads whose labels differ (clm_logit_deviation: a non-finite logit is sticky +inf).  Synchronises `st`.
template <class H>
int logits_deviation(H* h, hipStream_t st, const float* pair, int B, float* max_abs_diff, int* labels_differ) {
    std::vector<float> host((size_t)2 * B * NCLS);
    HIPCHK(h, hipMemcpyAsync(host.data(), pair, host.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    (void)clm_logit_deviation(host.data(), host.data() + (size_t)B * NCLS, B, NCLS, max_abs_diff, labels_differ);
    return CLM_OK;
}

// Profiling taps of a handle with N stages: HIP events on the launch stream around each stage span (StageTimer), summed per stage
// by read().  Events are reused from read to read; past MAX_RECORDS unread spans nothing more is recorded.
template <int N>
class StageProfile {
  public:
    static constexpr size_t MAX_RECORDS = 200000;
    StageProfile() = default;
    StageProfile(const StageProfile&) = delete;
    StageProfile& operator=(const StageProfile&) = delete;
    ~StageProfile() {
        for (auto& r : recs_) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        for (auto& e : free_) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    }
    bool begin(hipStream_t st, hipEvent_t& e0, hipEvent_t& e1) {          // false: this span is not recorded
        if (recs_.size() > MAX_RECORDS) return false;
        if (!free_.empty()) {
            e0 = free_.back().first;
            e1 = free_.back().second;
            free_.pop_back();
        } else if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            return false;
        }
        (void)hipEventRecord(e0, st);
        return true;
    }
    void end(int stage, hipEvent_t e0, hipEvent_t e1, hipStream_t st) {
        (void)hipEventRecord(e1, st);
        recs_.push_back({stage, e0, e1});
    }
    // totals per stage into ms_out / n_out ([N] each, or null); the caller has synchronised the device
    void read(double* ms_out, int64_t* n_out, bool reset) {
        for (auto& r : recs_) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
                ms_[r.stage] += ms;
                n_[r.stage] += 1;
            }
            free_.push_back({r.e0, r.e1});
        }
        recs_.clear();
        for (int i = 0; i < N; ++i) {
            if (ms_out) ms_out[i] = ms_[i];
            if (n_out) n_out[i] = n_[i];
            if (reset) { ms_[i] = 0; n_[i] = 0; }
        }
    }

  private:
    struct Rec {
        int stage;
        hipEvent_t e0, e1;
    };
    std::vector<Rec> recs_;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_;
    double ms_[N] = {};
    int64_t n_[N] = {};
};
// RAII: one span of `stage` on `st` while the handle's run mode asks for profiling (h->run.prof, h->profile)
template <class H>
struct StageTimer {
    H* h;
    hipStream_t st;
    int stage;
    hipEvent_t e0{}, e1{};
    bool on;
    StageTimer(H* h_, hipStream_t st_, int stage_) : h(h_), st(st_), stage(stage_), on(h_->run.prof && h_->profile.begin(st_, e0, e1)) {}
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() {
        if (on) h->profile.end(stage, e0, e1, st);
    }
};

// ---- SequenceCNNTransformer: what tf_model.hip and tf_fp32.hip share on the host ---------------------------------------------------
struct TfPacking {                // one packing of the matrices the MFMA kernels read (16-bit mode, t32 or x3)
    std::vector<std::array<DevBuf, 4>> mat;   // per layer
    DevBuf conv[3];                           // stem convolutions: three taps [dk][co][ci], each tap packed
};
// tf_fp32.hip: the forward with exact-fp32 products (the reference's precision; x3: on hi + lo halfs), up to the encoder output h.
// Launches only: false, and nothing launched behind it, where the attention refuses the shape (launch_attention_exact); a launch
// error is the caller's to read (launched)
size_t tf32_workspace_floats(int B, int L);
bool tf32_forward(const unsigned char* ids8, int ids_stride, int B, int L, int n_layers, float* ws, float* h, const TfNetF32& net,
                  const TfLayerF32* lay, const TfPacking& pk /*t32, or x3's*/, hipStream_t st, bool unfused, bool x3, int stop_after = -1);

}  // namespace clm
