// cnn.hip -- DNAConvNet forward on MI355X: kernels + engine + C ABI (clm_cnn_*).
//
// Reference: /root/reference/chimeralm/models/components/cnn.py (configured by configs/model/cnn.yaml: vocab 12, embedding 256,
// num_filters [256, 256, 256], kernel_sizes [7, 7, 7], pool_sizes [4, 4, 4], hidden 512, 2 classes), eval mode:
//   x = Embedding(12, 256)(ids)                         pads are ordinary tokens, no mask
//   3 x [Conv1d(256, 256, 7, padding "same"), BatchNorm1d (running stats), GELU (erf), MaxPool1d(4), Dropout]   L -> L/4 -> L/16 -> L/64
//   AdaptiveAvgPool1d(1) ; Linear(256, 512), BatchNorm1d, GELU, Dropout, Linear(512, 2)
//
// Four launches per batch (ids -> clamped bytes, then):
//   block 0   cnn_block0_kernel: the input is an embedding of 12 ids, so conv(embed(x))[t] = b + sum_dk T[dk][x[t + dk - 3]] with the
//             table T[dk][tok] = W[:, :, dk] . E[tok] (7 x 12 x 256 floats, computed in fp64 at finalize, held in LDS); a position
//             outside the read contributes nothing (row 12 of the LDS table is zero -- not E[4]: a loaded pad row need not be zero).
//             Bias, BatchNorm, GELU on each of the 4 positions of a window, then the max; writes [B, L/4, 256] fp32.
//   block 1   cnn_gemm7_kernel (tail32.hip): implicit GEMM, K = 7 x 256, on the fp32 MFMA or as fp16x3; writes [B, L/16, 256].
//   block 2   the same kernel; instead of its rows, per-64-row-tile channel sums of its pooled rows -> [B, tiles, 256].
//   head      cnn_head_kernel: the tiles' sums in a fixed order / (L/64), fc.0, BatchNorm, GELU, fc.4 -> logits [B, 2].
// No atomics: every reduction has a fixed order, so the forward is bitwise deterministic and a read's logits do not depend on the
// batch it is in.  BatchNorm is applied as y = x * scale + shift with scale = g / sqrt(var + eps), shift = b - mean * scale, both
// computed in fp64 at finalize (not folded into the weights).
// The net's constants and block 0's two staging steps are cnn_common.h's, shared with cnn_train.hip (and tail32.hip's cnn_gemm7_kernel).
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "chimeralm_hip.h"
#include "handle_host.h"
#include "cnn_common.h"

namespace clm {
namespace cnn {                    // (VOC, K, HALO, TROWS, BN_EPS and block 0's staging: cnn_common.h)

constexpr int HID = 512;           // fc hidden
constexpr int PT0 = 128;           // block 0: pooled positions per workgroup (512 tokens)
constexpr int ROWS2 = 16;          // block 2: pooled rows per 64-row tile of cnn_gemm7_kernel

// ------------------------------------------------------------------------------------------------ block 0
// grid (tiles, B), 512 threads: thread = (channel tid & 255, half tid >> 8 of the tile's pooled positions).
__global__ __launch_bounds__(512) void cnn_block0_kernel(const unsigned char* __restrict__ ids8, int Lp, const float* __restrict__ table,
                                                         const float* __restrict__ bias, const float* __restrict__ bn_scale,
                                                         const float* __restrict__ bn_shift, float* __restrict__ out, int L) {
    extern __shared__ __attribute__((aligned(16))) float smem_c0[];
    float* Ts = smem_c0;                                       // [K][TROWS][256]
    int* idl = reinterpret_cast<int*>(Ts + K * TROWS * D);     // [4 PT0 + 2 HALO]: LDS row of token 4 p0 - 3 + i
    const int tid = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * PT0, L4 = L / 4;
    stage_table(Ts, table, tid);
    stage_token_rows(idl, ids8 + (size_t)b * Lp, 4 * p0 - HALO, 4 * PT0 + 2 * HALO, L, tid, 1);
    __syncthreads();
    const int c = tid & (D - 1), half = tid >> 8;
    const float bc = bias[c], sc = bn_scale[c], sh = bn_shift[c];
    const float* Tc = Ts + c;
    const int pend = p0 + PT0 < L4 ? p0 + PT0 : L4;
#pragma unroll 1
    for (int p = p0 + half * (PT0 / 2); p < pend && p < p0 + (half + 1) * (PT0 / 2); ++p) {
        const int* id = idl + 4 * (p - p0);                    // token 4 p + j + dk - 3  ->  id[j + dk]
        int r[4 + K - 1];
#pragma unroll
        for (int i = 0; i < 4 + K - 1; ++i) r[i] = id[i] * D;
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = bc;
#pragma unroll
            for (int dk = 0; dk < K; ++dk) v += Tc[dk * TROWS * D + r[j + dk]];
            m = fmaxf(m, gelu_erf(v * sc + sh));
        }
        out[((size_t)b * L4 + p) * D + c] = m;
    }
}

// ------------------------------------------------------------------------------------------------ head
// one workgroup of 512 threads per read: mean of block 2's pooled rows, fc.0 (weights transposed [256][512]: coalesced), BN, GELU,
// fc.4; fixed reduction orders throughout
__global__ __launch_bounds__(512) void cnn_head_kernel(const float* __restrict__ partial, int tiles, int L64, const float* __restrict__ w0t,
                                                       const float* __restrict__ b0, const float* __restrict__ s1, const float* __restrict__ h1,
                                                       const float* __restrict__ w4, const float* __restrict__ b4, float* __restrict__ pooled,
                                                       float* __restrict__ logits) {
    __shared__ float P[D];
    __shared__ float red[2][8];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < D) {
        const float* src = partial + (size_t)b * tiles * D + tid;
        float s = 0.f;
        for (int i = 0; i < tiles; ++i) s += src[(size_t)i * D];
        s = s / (float)L64;
        P[tid] = s;
        pooled[(size_t)b * D + tid] = s;
    }
    __syncthreads();
    float a = b0[tid];
#pragma unroll 8
    for (int c = 0; c < D; ++c) a = fmaf(w0t[(size_t)c * HID + tid], P[c], a);
    const float g = gelu_erf(a * s1[tid] + h1[tid]);
    const float r0 = wave_sum(g * w4[tid]), r1 = wave_sum(g * w4[HID + tid]);
    if (lane == 0) {
        red[0][wave] = r0;
        red[1][wave] = r1;
    }
    __syncthreads();
    if (tid < NCLS) {
        const float* r = red[tid];
        logits[(size_t)b * NCLS + tid] = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + b4[tid];
    }
}

}  // namespace cnn
}  // namespace clm

// ================================================================================================ engine + C ABI
using namespace clm;

// Weights as the kernels take them: device pointers resolved ONCE, by clm_cnn_finalize, and what it computes from the rest
struct CnnF32 {                   // tensors the forward reads as loaded, fp32
    const float *conv_b[3], *fc0_b, *fc4_w, *fc4_b;
};
struct CnnBn {                    // BatchNorm1d in eval mode as y = x * scale + shift
    DevBuf scale, shift;
};
struct CnnDev {                   // finalize products
    DevBuf table;                 // block 0: T[dk][tok][co]
    DevBuf conv1, conv2;          // blocks 1 and 2: seven taps [dk][co][ci], each tap packed (f32t, or x3 halfs: x3_active)
    CnnBn bn[4];                  // blocks 0 .. 2, fc.1
    DevBuf fc0t;                  // fc.0.weight transposed [256][512]
};

struct clm_cnn_handle {
    int device = 0;
    bool x3 = false;                              // CLM_PREC_F16X3 handle
    bool x3_active = false;                       // ... and its block 1 / 2 weights are inside the packing's range (finalize)
    std::string err;
    std::map<std::string, DevBuf> w;              // fp32 device copies by reference key
    WeightTable expected;                         // (clm_cnn_create)
    CnnF32 f = {};
    CnnDev dev;
    bool finalized = false;
    DevBuf ids8, x1, x2, part, pooled;            // workspace (clm_cnn_forward)
    int last_B = 0, last_L = 0;
};

namespace {

// clm_cnn_create: the state-dict keys, their shapes and the field of h->f the forward reads each from (none: finalize alone reads it)
void cnn_expect(clm_cnn_handle* h) {
    WeightTable& e = h->expected;
    e["embedding.weight"] = {{cnn::VOC, D}, nullptr};
    for (int i = 0; i < 3; ++i) {
        const std::string p = "conv_blocks." + std::to_string(i) + ".";
        e[p + "0.weight"] = {{D, D, cnn::K}, nullptr}; e[p + "0.bias"] = {{D}, &h->f.conv_b[i]};
        for (const char* s : {"weight", "bias", "running_mean", "running_var"}) e[p + "1." + s] = {{D}, nullptr};
    }
    e["fc.0.weight"] = {{cnn::HID, D}, nullptr}; e["fc.0.bias"] = {{cnn::HID}, &h->f.fc0_b};
    for (const char* s : {"weight", "bias", "running_mean", "running_var"}) e[std::string("fc.1.") + s] = {{cnn::HID}, nullptr};
    e["fc.4.weight"] = {{NCLS, cnn::HID}, &h->f.fc4_w}; e["fc.4.bias"] = {{NCLS}, &h->f.fc4_b};
}

bool is_batches_tracked(const std::string& k) {
    const std::string s = "num_batches_tracked";
    return k.size() >= s.size() && k.compare(k.size() - s.size(), s.size(), s) == 0;
}

int cnn_host(clm_cnn_handle* h, const std::string& k, std::vector<float>& out) { return host_f32(h, "clm_cnn_finalize", k, out); }

// BatchNorm1d in eval mode as scale / shift, computed in fp64 and rounded once
int cnn_bn(clm_cnn_handle* h, const std::string& p, CnnBn& bn, int n) {
    std::vector<float> g, b, m, v;
    int rc;
    if ((rc = cnn_host(h, p + "weight", g)) || (rc = cnn_host(h, p + "bias", b)) || (rc = cnn_host(h, p + "running_mean", m)) ||
        (rc = cnn_host(h, p + "running_var", v)))
        return rc;
    std::vector<float> sc(n), sh(n);
    for (int i = 0; i < n; ++i) {
        const double s = (double)g[i] / std::sqrt((double)v[i] + (double)cnn::BN_EPS);
        sc[i] = (float)s;
        sh[i] = (float)((double)b[i] - (double)m[i] * s);
    }
    if ((rc = upload_f32(h, bn.scale, sc))) return rc;
    return upload_f32(h, bn.shift, sh);
}

}  // namespace

extern "C" {

int clm_cnn_create(int device, int precision, clm_cnn_handle** out) {
    if (!out) return fail<clm_cnn_handle>(nullptr, CLM_E_INVALID, "clm_cnn_create: bad argument");
    if (precision != CLM_PREC_F32 && precision != CLM_PREC_F16X3)
        return fail<clm_cnn_handle>(nullptr, CLM_E_INVALID, "clm_cnn_create: precision must be CLM_PREC_F32 (exact) or CLM_PREC_F16X3");
    if (int rc = use_gfx950<clm_cnn_handle>(device, "clm_cnn_create")) return rc;
    clm_cnn_handle* h = new clm_cnn_handle();
    h->device = device;
    h->x3 = precision == CLM_PREC_F16X3;
    cnn_expect(h);
    *out = h;
    return CLM_OK;
}

int clm_cnn_load_weight(clm_cnn_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !key || !data || !shape || ndim < 0) return fail(h, CLM_E_INVALID, "clm_cnn_load_weight: null argument");
    const std::string k = canonical_weight_key(key);
    if (is_batches_tracked(k)) return CLM_OK;                  // BatchNorm's step counter: not used in eval mode
    if (dtype != CLM_DT_F32) return fail(h, CLM_E_INVALID, "clm_cnn_load_weight: fp32 tensors only");
    return load_f32(h, "clm_cnn_load_weight", k, data, shape, ndim);
}

int clm_cnn_finalize(clm_cnn_handle* h) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = resolve_weights(h, "clm_cnn_finalize")) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    h->dev = CnnDev{};
    h->finalized = false;
    int rc;
    // block 0's table T[dk][tok][co] = sum_ci W[co][ci][dk] E[tok][ci], in fp64
    {
        std::vector<float> E, W;
        if ((rc = cnn_host(h, "embedding.weight", E)) || (rc = cnn_host(h, "conv_blocks.0.0.weight", W))) return rc;
        std::vector<float> T((size_t)cnn::K * cnn::VOC * D);
        for (int dk = 0; dk < cnn::K; ++dk)
            for (int tok = 0; tok < cnn::VOC; ++tok)
                for (int co = 0; co < D; ++co) {
                    double s = 0.0;
                    for (int ci = 0; ci < D; ++ci) s += (double)W[((size_t)co * D + ci) * cnn::K + dk] * (double)E[(size_t)tok * D + ci];
                    T[((size_t)dk * cnn::VOC + tok) * D + co] = (float)s;
                }
        if ((rc = upload_f32(h, h->dev.table, T))) return rc;
    }
    // blocks 1 and 2: [co][ci][dk] -> seven taps [co][ci], each packed for the MFMA.  fp16x3 packs w x 2^10 as fp16 hi + lo, which
    // saturates for |w| >= 64: such weights run in the exact-fp32 packing instead (chimeralm_amd/cnn.py reports it)
    std::vector<std::vector<float>> Wb(2);
    float wmax = 0.f;
    for (int i = 1; i <= 2; ++i) {
        if ((rc = cnn_host(h, "conv_blocks." + std::to_string(i) + ".0.weight", Wb[i - 1]))) return rc;
        for (float v : Wb[i - 1]) wmax = std::fmax(wmax, std::fabs(v));
    }
    h->x3_active = h->x3 && wmax < X3_WEIGHT_LIMIT;
    {
        DevBuf split;
        std::vector<float> hs((size_t)cnn::K * D * D);
        for (int i = 1; i <= 2; ++i) {
            const std::vector<float>& W = Wb[i - 1];
            for (int dk = 0; dk < cnn::K; ++dk)
                for (int co = 0; co < D; ++co)
                    for (int ci = 0; ci < D; ++ci) hs[((size_t)dk * D + co) * D + ci] = W[((size_t)co * D + ci) * cnn::K + dk];
            if ((rc = upload_f32(h, split, hs))) return rc;
            auto pack = [&](const float* tap, void* out) {
                if (h->x3_active) launch_pack_x3(tap, out, D, D, 0);
                else launch_pack_f32t(tap, out, D, D, 0);
            };
            if ((rc = pack_taps(h, split.get<float>(), cnn::K, (size_t)D * D * 4, i == 1 ? h->dev.conv1 : h->dev.conv2, pack))) return rc;   // (synchronised: `split` is reused)
        }
    }
    for (int i = 0; i < 3; ++i)
        if ((rc = cnn_bn(h, "conv_blocks." + std::to_string(i) + ".1.", h->dev.bn[i], D))) return rc;
    if ((rc = cnn_bn(h, "fc.1.", h->dev.bn[3], cnn::HID))) return rc;
    {
        std::vector<float> W0;
        if ((rc = cnn_host(h, "fc.0.weight", W0))) return rc;
        if ((rc = upload_f32(h, h->dev.fc0t, transposed(W0, cnn::HID, D)))) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    return CLM_OK;
}

int clm_cnn_forward(clm_cnn_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                    void* stream) {
    if (!h) return CLM_E_INVALID;
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_cnn_forward before clm_cnn_finalize");
    // (64 tokens: three max-pools of 4; the reference raises 'Invalid computed output size: 0' below that)
    if (int rc = check_ids_arg(h, "clm_cnn_forward", ids, logits_out, ids_dtype, ids_row_stride, B, L, 64)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int Lp = (L + 63) / 64 * 64, L4 = L / 4, L16 = L4 / 4, L64 = L16 / 4;
    const int tiles2 = (L64 + cnn::ROWS2 - 1) / cnn::ROWS2;
    if (int rc = grow(h, Sync::Device(), {{&h->ids8, (size_t)B * Lp}, {&h->x1, (size_t)B * L4 * D * 4}, {&h->x2, (size_t)B * L16 * D * 4},
                                          {&h->part, (size_t)B * tiles2 * D * 4}, {&h->pooled, (size_t)B * D * 4}}))
        return rc;
    const CnnF32& f = h->f;
    const CnnDev& dv = h->dev;
    unsigned char* const ids8 = h->ids8.get<unsigned char>();
    float *const x1 = h->x1.get<float>(), *const x2 = h->x2.get<float>(), *const part = h->part.get<float>();
    launch_embed(ids, ids_dtype, ids_row_stride, nullptr, nullptr, ids8, B, L, Lp, st);   // ids of any dtype -> clamped bytes
    {
        const size_t lds = (size_t)cnn::K * cnn::TROWS * D * 4 + (size_t)(4 * cnn::PT0 + 2 * cnn::HALO) * 4;
        launch_lds<cnn::cnn_block0_kernel>(dim3((unsigned)((L4 + cnn::PT0 - 1) / cnn::PT0), (unsigned)B), dim3(512), lds, st, ids8, Lp,
                                           dv.table.get<float>(), f.conv_b[0], dv.bn[0].scale.get<float>(), dv.bn[0].shift.get<float>(), x1, L);
    }
    launch_cnn_gemm7(x1, dv.conv1.get<float>(), f.conv_b[1], dv.bn[1].scale.get<float>(), dv.bn[1].shift.get<float>(), x2, false, B, L4, st,
                     h->x3_active);
    launch_cnn_gemm7(x2, dv.conv2.get<float>(), f.conv_b[2], dv.bn[2].scale.get<float>(), dv.bn[2].shift.get<float>(), part, true, B, L16, st,
                     h->x3_active);
    hipLaunchKernelGGL(cnn::cnn_head_kernel, dim3((unsigned)B), dim3(512), 0, st, part, tiles2, L64, dv.fc0t.get<float>(), f.fc0_b,
                       dv.bn[3].scale.get<float>(), dv.bn[3].shift.get<float>(), f.fc4_w, f.fc4_b, h->pooled.get<float>(), logits_out);
    h->last_B = B; h->last_L = L;
    return launched(h, "clm_cnn_forward");
}

int clm_cnn_debug_fetch(clm_cnn_handle* h, const char* name, void* host_out, size_t bytes) {
    if (!h || !name || !host_out) return fail(h, CLM_E_INVALID, "clm_cnn_debug_fetch: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const std::string n(name);
    const size_t B = (size_t)h->last_B, L4 = (size_t)(h->last_L / 4), L16 = L4 / 4, L64 = L16 / 4;
    const void* src = nullptr;
    size_t have = 0;
    if (n == "block0") { src = h->x1.get(); have = B * L4 * D * 4; }
    else if (n == "block1") { src = h->x2.get(); have = B * L16 * D * 4; }
    else if (n == "partial") { src = h->part.get(); have = B * ((L64 + cnn::ROWS2 - 1) / cnn::ROWS2) * D * 4; }
    else if (n == "pooled") { src = h->pooled.get(); have = B * D * 4; }
    else return fail(h, CLM_E_INVALID, "clm_cnn_debug_fetch: unknown name " + n);
    return fetch_bytes(h, "clm_cnn_debug_fetch", n, src, have, host_out, bytes);
}

const char* clm_cnn_last_error(const clm_cnn_handle* h) { return h ? h->err.c_str() : create_error<clm_cnn_handle>().c_str(); }

int clm_cnn_destroy(clm_cnn_handle* h) { return destroy_handle(h); }

}  // extern "C"
