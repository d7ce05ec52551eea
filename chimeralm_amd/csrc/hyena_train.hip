// hyena_train.hip -- the core of the Hyena operator for training, forward and backward, exact fp32:
//   u_r[t] = sb[r] + sum_j sw[r, j] zc[r, t - 2 + j]            r = ch, 256 + ch, 512 + ch  ->  x0, x1, v
//   g = v x1        c = causal_conv(g, k[ch]) + D[ch] g        y = c x0
// and, given dy and the saved c (g, x0, x1, v are recomputed from zc):
//   dc = dy x0      dx0 = dy c      dg[s] = sum_{t >= s} dc[t] k[t - s] + D dc[s]
//   dk[ch, tau] = sum_b sum_{t >= tau} dc[b, t] g[b, t - tau]          dD[ch] = sum_{b, t} dc g
//   dx1 = dg v      dv = dg x1      dzc, dsw, dsb: the transpose of the 3-tap filter.
//
// Transform form.  N = 2^logn >= 2 L - 2 (conv_logn_for), the LDS Stockham passes of fft_passes.h.  Every transform packs TWO REAL
// SEQUENCES OF ONE READ as real and imaginary part and separates their spectra through the mirrored bin,
//   A[m] = (Z[m] + conj Z[N - m]) / 2,   B[m] = (Z[m] - conj Z[N - m]) / 2i,
// so that no result of a read meets another read's numbers (packing two READS, as the inference kernel does, makes a read's
// rounding depend on its partner):
//   forward   z = g[ch] + i g[ch + 1] (two channels of a read)      W = A K[ch] + i B K[ch + 1]            IFFT(W) = c[ch] + i c[ch + 1]
//   backward  z = dc + i g (one channel of a read)                  W = A conj K + i A conj B              IFFT(W) = dg + i dk_read
// W[N - m] = conj S1[m] + i conj S2[m] because both products are spectra of real sequences.  The per-read dk rows go to the
// workspace and are added in read order by hyena_train_reduce_kernel.  N == 2 L - 2 wraps exactly one product into each result:
//   c[0] -= g[L-1] k[L-1]      dg[L-1] -= dc[0] k[L-1]      dk_read[L-1] -= dc[0] g[L-1].
// No floating-point atomics anywhere; every sum has one fixed order.
#include "hyena_train_blocks.h"

namespace clm {
using namespace clmfft;

namespace {

struct HtLayout {                                 // the workspace, in floats (include/chimeralm_hip.h states the same sum)
    size_t tw, kf, dkp, part, total;
    HtLayout(int B, int L, int logn) {
        const size_t N = (size_t)1 << logn, H = N / 2 + 1;
        tw = 0;                                   // exp(-2 pi i m / N), m < N / 2
        kf = tw + N;                              // FFT(k[ch]) / N, bins 0 .. N / 2, per channel
        dkp = kf + 2 * D * H;                     // dk of each read [B, 256, L]
        part = dkp + (size_t)B * D * L;           // parameter partials [B, 256, 16]
        total = part + (size_t)B * D * HT_PART;
    }
};

__global__ __launch_bounds__(256) void hyena_train_twiddle_kernel(float2* __restrict__ tw, int logn) {
    const int m = blockIdx.x * 256 + threadIdx.x, N = 1 << logn;
    if (m < N / 2) {
        double sn, cs;
        sincospi(-2.0 * (double)m / (double)N, &sn, &cs);
        tw[m] = make_float2((float)cs, (float)sn);
    }
}

// K[ch][m] = FFT(k[ch])[m] / N for m = 0 .. N / 2 (k is real: the other bins are the conjugates), once per call
template <int LOGN>
__global__ __launch_bounds__(Plan<LOGN>::NT) void hyena_train_spectrum_kernel(const float* __restrict__ k, float2* __restrict__ kf,
                                                                              const float2* __restrict__ tw, int L) {
    constexpr int N = 1 << LOGN, NT = Plan<LOGN>::NT, H = N / 2 + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(N);
    const int tid = threadIdx.x, ch = blockIdx.x;
    const float* kr = k + (size_t)ch * L;
    for (int t = tid; t < N; t += NT) {
        re[pad_index(t)] = t < L ? kr[t] : 0.f;
        im[pad_index(t)] = 0.f;
    }
    __syncthreads();
    hyena_train_fft<LOGN, false>(re, im, tid, tw);
    const float inv = 1.0f / (float)N;
    for (int m = tid; m < H; m += NT) kf[(size_t)ch * H + m] = make_float2(re[pad_index(m)] * inv, im[pad_index(m)] * inv);
}

// One workgroup = (channel pair, read).
template <int LOGN>
__global__ __launch_bounds__(Plan<LOGN>::NT) void hyena_train_fwd_kernel(const float* __restrict__ zc, const float* __restrict__ sw,
                                                                         const float* __restrict__ sb, const float* __restrict__ k,
                                                                         const float* __restrict__ Dk, const float2* __restrict__ kf,
                                                                         const float2* __restrict__ tw, float* __restrict__ c,
                                                                         float* __restrict__ y, int L) {
    constexpr int N = 1 << LOGN, NT = Plan<LOGN>::NT, H = N / 2 + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(N);
    float* red = im + padded_size(N);
    const int tid = threadIdx.x, c0 = 2 * blockIdx.x, c1 = c0 + 1, b = blockIdx.y;
    const float* zb = zc + (size_t)b * D3 * L;
    HtShort s0, s1;
    s0.load(sw, sb, c0);
    s1.load(sw, sb, c1);

    float n0 = 0.f, n1 = 0.f;
    for (int t = tid; t < N; t += NT) {
        float g0 = 0.f, g1 = 0.f;
        if (t < L) {
            HtTaps a, e;
            hyena_train_taps(zb, c0, t, L, s0, a);
            hyena_train_taps(zb, c1, t, L, s1, e);
            g0 = a.u[2] * a.u[1];
            g1 = e.u[2] * e.u[1];
        }
        re[pad_index(t)] = g0;
        im[pad_index(t)] = g1;
        n0 = fmaf(g0, g0, n0);
        n1 = fmaf(g1, g1, n1);
    }
    const float2 nin = hyena_train_block_sum2<NT>(n0, n1, red, tid);
    const float rin = hyena_train_balance(nin.x, nin.y);
    hyena_train_scale_im<LOGN>(im, tid, L, rin);
    __syncthreads();
    hyena_train_fft<LOGN, false>(re, im, tid, tw);
    const float2* k0 = kf + (size_t)c0 * H;
    const float2* k1 = kf + (size_t)c1 * H;
    const float rout = hyena_train_products<LOGN>(re, im, red, tid, [&](float2 a2, float2 b2, int m, float2& p1, float2& p2) {
        const float2 ka = k0[m], kb = k1[m];
        p1 = cmul(make_float2(0.5f * a2.x, 0.5f * a2.y), ka);
        p2 = cmul(make_float2(0.5f * b2.x, 0.5f * b2.y), kb);
    });
    __syncthreads();
    hyena_train_fft<LOGN, true>(re, im, tid, tw);
    const float unscale = 1.0f / (rin * rout);                   // both powers of two: exact

    const bool alias = (2 * L - 2 == N);
    const float d0 = Dk[c0], d1 = Dk[c1];
    float* cr0 = c + ((size_t)b * D + c0) * L;
    float* yr0 = y + ((size_t)b * D + c0) * L;
    for (int t = tid; t < L; t += NT) {
        HtTaps a, e;
        hyena_train_taps(zb, c0, t, L, s0, a);
        hyena_train_taps(zb, c1, t, L, s1, e);
        float v0 = re[pad_index(t)], v1 = im[pad_index(t)] * unscale;
        if (alias && t == 0) {                    // the one wrapped product
            HtTaps la, le;
            hyena_train_taps(zb, c0, L - 1, L, s0, la);
            hyena_train_taps(zb, c1, L - 1, L, s1, le);
            v0 -= la.u[2] * la.u[1] * k[(size_t)c0 * L + L - 1];
            v1 -= le.u[2] * le.u[1] * k[(size_t)c1 * L + L - 1];
        }
        v0 = fmaf(d0, a.u[2] * a.u[1], v0);
        v1 = fmaf(d1, e.u[2] * e.u[1], v1);
        cr0[t] = v0;
        cr0[(size_t)L + t] = v1;
        yr0[t] = v0 * a.u[0];
        yr0[(size_t)L + t] = v1 * e.u[0];
    }
}

// One workgroup = (channel, read).
template <int LOGN>
__global__ __launch_bounds__(Plan<LOGN>::NT) void hyena_train_bwd_kernel(const float* __restrict__ zc, const float* __restrict__ sw,
                                                                         const float* __restrict__ sb, const float* __restrict__ k,
                                                                         const float* __restrict__ Dk, const float* __restrict__ c,
                                                                         const float* __restrict__ dy, const float2* __restrict__ kf,
                                                                         const float2* __restrict__ tw, float* __restrict__ dzc,
                                                                         float* __restrict__ dkp, float* __restrict__ part, int L) {
    constexpr int N = 1 << LOGN, NT = Plan<LOGN>::NT, H = N / 2 + 1, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(N);
    float* red = im + padded_size(N);             // [NW][HT_PART]
    const int tid = threadIdx.x, ch = blockIdx.x, b = blockIdx.y;
    const float* zb = zc + (size_t)b * D3 * L;
    const float* cr = c + ((size_t)b * D + ch) * L;
    const float* dyr = dy + ((size_t)b * D + ch) * L;
    HtShort s;
    s.load(sw, sb, ch);

    float nd = 0.f, ng = 0.f;
    for (int t = tid; t < N; t += NT) {           // z = dc + i g
        float dc = 0.f, g = 0.f;
        if (t < L) {
            HtTaps a;
            hyena_train_taps(zb, ch, t, L, s, a);
            dc = dyr[t] * a.u[0];
            g = a.u[2] * a.u[1];
        }
        re[pad_index(t)] = dc;
        im[pad_index(t)] = g;
        nd = fmaf(dc, dc, nd);
        ng = fmaf(g, g, ng);
    }
    const float2 nin = hyena_train_block_sum2<NT>(nd, ng, red, tid);
    const float rin = hyena_train_balance(nin.x, nin.y);
    hyena_train_scale_im<LOGN>(im, tid, L, rin);
    __syncthreads();
    hyena_train_fft<LOGN, false>(re, im, tid, tw);
    const float2* kc = kf + (size_t)ch * H;
    const float qn = 0.25f / (float)N;
    const float rout = hyena_train_products<LOGN>(re, im, red, tid, [&](float2 a2, float2 b2, int m, float2& p1, float2& p2) {
        p1 = cmul(make_float2(0.5f * a2.x, 0.5f * a2.y), cconj(kc[m]));     // FFT(dc) conj K / N
        p2 = cmul(make_float2(qn * a2.x, qn * a2.y), cconj(b2));            // FFT(dc) conj FFT(rin g) / N
    });
    __syncthreads();
    hyena_train_fft<LOGN, true>(re, im, tid, tw);    // re = dg (without the skip term), im = this read's dk times rin rout
    const float unscale = 1.0f / (rin * rout);       // both powers of two: exact

    const bool alias = (2 * L - 2 == N);
    const float dskip = Dk[ch];
    float acc[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) acc[j] = 0.f;
    float* dkr = dkp + ((size_t)b * D + ch) * L;
    for (int t = tid; t < N; t += NT) {           // planes become dx1 | dv (zero from L on, for the transposed taps)
        float dx1 = 0.f, dv = 0.f;
        if (t < L) {
            HtTaps a;
            hyena_train_taps(zb, ch, t, L, s, a);
            const float dyt = dyr[t], dc = dyt * a.u[0], g = a.u[2] * a.u[1], dx0 = dyt * cr[t];
            float dg = re[pad_index(t)], dkt = im[pad_index(t)] * unscale;
            if (alias && t == L - 1) {
                HtTaps f;
                hyena_train_taps(zb, ch, 0, L, s, f);
                const float dc0 = dyr[0] * f.u[0];
                dg -= dc0 * k[(size_t)ch * L + L - 1];
                dkt -= dc0 * g;
            }
            dkr[t] = dkt;
            dg = fmaf(dskip, dc, dg);
            dx1 = dg * a.u[2];
            dv = dg * a.u[1];
            const float du[3] = {dx0, dx1, dv};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
#pragma unroll
                for (int e = 0; e < 3; ++e) acc[q * 3 + e] = fmaf(du[q], a.z[q][e], acc[q * 3 + e]);
                acc[9 + q] += du[q];
            }
            acc[12] = fmaf(dc, g, acc[12]);
        }
        if (t < L + 2) {
            re[pad_index(t)] = dx1;
            im[pad_index(t)] = dv;
        }
    }
    __syncthreads();
    float* dz0 = dzc + ((size_t)b * D3 + ch) * L;
    for (int t = tid; t < L; t += NT) {           // dzc[r, t] = sw[r, 2] du[t] + sw[r, 1] du[t + 1] + sw[r, 0] du[t + 2]
        float dx0[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) dx0[e] = t + e < L ? dyr[t + e] * cr[t + e] : 0.f;
        const float* planes[2] = {re, im};
        dz0[t] = fmaf(s.w[0][0], dx0[2], fmaf(s.w[0][1], dx0[1], s.w[0][2] * dx0[0]));
#pragma unroll
        for (int q = 1; q < 3; ++q) {
            const float* p = planes[q - 1];
            dz0[(size_t)q * D * L + t] =
                fmaf(s.w[q][0], p[pad_index(t + 2)], fmaf(s.w[q][1], p[pad_index(t + 1)], s.w[q][2] * p[pad_index(t)]));
        }
    }
    // the row's partials: lanes in wave_sum's order, then waves in wave order
#pragma unroll
    for (int j = 0; j < 13; ++j) {
        const float w = wave_sum(acc[j]);
        if ((tid & 63) == 0) red[(tid >> 6) * HT_PART + j] = w;
    }
    __syncthreads();
    if (tid < 13) {
        float sum = 0.f;
        for (int w = 0; w < NW; ++w) sum += red[w * HT_PART + tid];
        part[((size_t)b * D + ch) * HT_PART + tid] = sum;
    }
}

// dk[ch, t] = sum over reads in read order; block (x = 0) of a channel also adds its parameter partials in read order
__global__ __launch_bounds__(256) void hyena_train_reduce_kernel(const float* __restrict__ dkp, const float* __restrict__ part,
                                                                 float* __restrict__ dk, float* __restrict__ dsw, float* __restrict__ dsb,
                                                                 float* __restrict__ dD, int B, int L) {
    const int ch = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t < L) {
        float sum = 0.f;
        for (int b = 0; b < B; ++b) sum += dkp[((size_t)b * D + ch) * L + t];
        dk[(size_t)ch * L + t] = sum;
    }
    if (blockIdx.x == 0 && threadIdx.x < 13) {
        const int j = threadIdx.x;
        float sum = 0.f;
        for (int b = 0; b < B; ++b) sum += part[((size_t)b * D + ch) * HT_PART + j];
        if (j < 9) dsw[((j / 3) * D + ch) * 3 + j % 3] = sum;
        else if (j < 12) dsb[(j - 9) * D + ch] = sum;
        else dD[ch] = sum;
    }
}

template <int LOGN>
size_t ht_lds() { return (size_t)(2 * padded_size(1 << LOGN) + (Plan<LOGN>::NT / 64) * HT_PART) * sizeof(float); }

template <int LOGN>
void ht_prepare(const float* k, float* ws, const HtLayout& lay, int L, hipStream_t st) {
    float2* tw = reinterpret_cast<float2*>(ws + lay.tw);
    hipLaunchKernelGGL(hyena_train_twiddle_kernel, dim3(((1 << LOGN) / 2 + 255) / 256), dim3(256), 0, st, tw, LOGN);
    launch_lds<hyena_train_spectrum_kernel<LOGN>>(dim3(D), dim3(Plan<LOGN>::NT), ht_lds<LOGN>(), st, k, reinterpret_cast<float2*>(ws + lay.kf),
                                                  (const float2*)tw, L);
}

template <int LOGN>
void ht_forward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk, int B, int L, float* c, float* y,
                float* ws, hipStream_t st) {
    const HtLayout lay(B, L, LOGN);
    ht_prepare<LOGN>(k, ws, lay, L, st);
    launch_lds<hyena_train_fwd_kernel<LOGN>>(dim3(D / 2, B), dim3(Plan<LOGN>::NT), ht_lds<LOGN>(), st, zc, sw, sb, k, Dk,
                                             (const float2*)reinterpret_cast<float2*>(ws + lay.kf),
                                             (const float2*)reinterpret_cast<float2*>(ws + lay.tw), c, y, L);
}

template <int LOGN>
void ht_backward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk, const float* c, const float* dy, int B,
                 int L, float* dzc, float* dsw, float* dsb, float* dk, float* dD, float* ws, hipStream_t st) {
    const HtLayout lay(B, L, LOGN);
    ht_prepare<LOGN>(k, ws, lay, L, st);
    launch_lds<hyena_train_bwd_kernel<LOGN>>(dim3(D, B), dim3(Plan<LOGN>::NT), ht_lds<LOGN>(), st, zc, sw, sb, k, Dk, c, dy,
                                             (const float2*)reinterpret_cast<float2*>(ws + lay.kf),
                                             (const float2*)reinterpret_cast<float2*>(ws + lay.tw), dzc, ws + lay.dkp, ws + lay.part, L);
    hipLaunchKernelGGL(hyena_train_reduce_kernel, dim3((L + 255) / 256, D), dim3(256), 0, st, (const float*)(ws + lay.dkp),
                       (const float*)(ws + lay.part), dk, dsw, dsb, dD, B, L);
}

// CLM_OK, or why the shape is refused
int ht_shape(int B, int L) {
    if (B < 1 || L < 1 || B > 65535) return CLM_E_INVALID;
    return conv_logn_for(L) < 0 ? CLM_E_UNSUPPORTED : CLM_OK;
}
bool ht_ptrs(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p || (reinterpret_cast<uintptr_t>(p) & 3)) return false;
    return true;
}

#define HT_DISPATCH(logn, FN, ...)                  \
    switch (logn) {                                 \
        case 8: FN<8>(__VA_ARGS__); break;          \
        case 9: FN<9>(__VA_ARGS__); break;          \
        case 10: FN<10>(__VA_ARGS__); break;        \
        case 11: FN<11>(__VA_ARGS__); break;        \
        case 12: FN<12>(__VA_ARGS__); break;        \
        case 13: FN<13>(__VA_ARGS__); break;        \
        default: FN<14>(__VA_ARGS__); break;        \
    }

}  // namespace

}  // namespace clm

using namespace clm;

extern "C" int64_t clm_hyena_train_workspace_bytes(int B, int L) {
    const int rc = ht_shape(B, L);
    if (rc != CLM_OK) return rc;
    return ((int64_t)HtLayout(B, L, conv_logn_for(L)).total * (int64_t)sizeof(float) + 15) & ~(int64_t)15;
}

extern "C" int clm_hyena_train_forward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk, int B, int L,
                                       float* c_out, float* y_out, void* workspace, void* stream) {
    const int rc = ht_shape(B, L);
    if (rc != CLM_OK) return rc;
    if (!ht_ptrs({zc, sw, sb, k, Dk, c_out, y_out, workspace})) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    HT_DISPATCH(conv_logn_for(L), ht_forward, zc, sw, sb, k, Dk, B, L, c_out, y_out, ws, st);
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}

extern "C" int clm_hyena_train_backward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk, const float* c,
                                        const float* dy, int B, int L, float* dzc, float* dsw, float* dsb, float* dk, float* dD,
                                        void* workspace, void* stream) {
    const int rc = ht_shape(B, L);
    if (rc != CLM_OK) return rc;
    if (!ht_ptrs({zc, sw, sb, k, Dk, c, dy, dzc, dsw, dsb, dk, dD, workspace})) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    HT_DISPATCH(conv_logn_for(L), ht_backward, zc, sw, sb, k, Dk, c, dy, B, L, dzc, dsw, dsb, dk, dD, ws, st);
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}
