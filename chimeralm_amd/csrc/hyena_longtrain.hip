// hyena_longtrain.hip -- the core of the Hyena operator for training on reads of up to 32,769 tokens, forward and backward, exact
// fp32: the operator of hyena_train.hip as a uniformly partitioned convolution over segments of
// P = 8192 tokens with transforms of N = 2 P points.  S = ceil(L / P); segment x_i[a] = x[i P + a], zero beyond L and outside
// 0 .. S - 1.  Overlap-save, so nothing is carried from one segment's transform to the next:
//   K_j  = FFT([k_j ; 0]) / N                       per channel, once per call (hyena_longtrain_spectrum_kernel)
//   X_i  = FFT([g_{i-1} ; g_i])                     c_i  = IFFT( sum_{j <= i} X_{i-j} K_j )[P .. 2 P)
//   W_m  = FFT([dc_m ; dc_{m+1}])                   G_m  = FFT([g_m ; 0])
//   dg_i = IFFT( sum_{j < S-i} W_{i+j} conj K_j )[0 .. P)
//   dk_i = IFFT( sum_{m < S-i} W_{m+i} conj G_m )[0 .. P) / N     per read; the reads are added in read order afterwards
//   c += D g    dg += D dc    dD, dx0, dx1, dv, dzc, dsw, dsb as in hyena_train.hip.
// No product wraps at N = 2 P: there is no alias correction.
//
// Packing is 5.15's: two real sequences of ONE read per transform, separated through the mirrored bin -- forward the same segment
// of two channels, backward [dc_m ; dc_{m+1}] + i r [g_m ; 0] of one channel, and for the results S1 + i r' S2 of the two
// accumulated product spectra, one inverse per segment.  r, r' are the powers of two of hyena_train_balance.  Separated spectra go
// to the workspace UNSCALED (divided by r before the store), so that the spectra of different segments add with no factor between
// them.  A thread owns the bin pairs (m, N - m), m = tid + 512 q, in every stage: it reads back from the workspace only what it
// wrote itself, and the products of a pair wait in the pair's own two LDS slots between the norm sums and the packing.
//
// One workgroup walks the segments of its (channel pair, read) or (channel, read) in a fixed order; every sum has one fixed order
// and there are no floating-point atomics.  A read's c, y and dzc depend on no other read.
#include "hyena_train_blocks.h"

namespace clm {
using namespace clmfft;

namespace {

constexpr int HL_LOGN = 14, HL_N = 1 << HL_LOGN, HL_P = HL_N / 2, HL_H = HL_N / 2 + 1, HL_NT = Plan<HL_LOGN>::NT;
constexpr int HL_MAX_TOKENS = 4 * HL_P + 1;       // 32769
static_assert(HL_NT == 512 && HL_P % HL_NT == 0, "a thread owns whole strides of a segment");

inline int hl_segments(int L) { return (L + HL_P - 1) / HL_P; }

struct HlLayout {                                 // the workspace, in floats (include/chimeralm_hip.h states the same sum)
    size_t tw, kf, spec, dkp, part, total;
    HlLayout(int B, int L) {
        const size_t S = (size_t)hl_segments(L);
        tw = 0;                                   // exp(-2 pi i m / N), m < N / 2
        kf = tw + HL_N;                           // K_j, bins 0 .. N / 2 [256, S, H] complex
        spec = kf + 2 * D * S * HL_H;             // segment spectra: backward W_m, G_m [B, 256, S, 2, H] complex; forward uses half
        dkp = spec + 4 * (size_t)B * D * S * HL_H;             // dk of each read [B, 256, L]
        part = dkp + (size_t)B * D * L;           // parameter partials [B, 256, 16]
        total = part + (size_t)B * D * HT_PART;
    }
};

__global__ __launch_bounds__(256) void hyena_longtrain_twiddle_kernel(float2* __restrict__ tw) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < HL_N / 2) {
        double sn, cs;
        sincospi(-2.0 * (double)m / (double)HL_N, &sn, &cs);
        tw[m] = make_float2((float)cs, (float)sn);
    }
}

// K_j[ch][m] = FFT([k_j ; 0])[m] / N for m = 0 .. N / 2.  Bins 0 and N / 2 of a real sequence are real: stored so.
__global__ __launch_bounds__(HL_NT) void hyena_longtrain_spectrum_kernel(const float* __restrict__ k, float2* __restrict__ kf,
                                                                         const float2* __restrict__ tw, int L, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(HL_N);
    const int tid = threadIdx.x, ch = blockIdx.x, j = blockIdx.y;
    const float* kr = k + (size_t)ch * L;
    for (int t = tid; t < HL_N; t += HL_NT) {
        const int tg = j * HL_P + t;
        re[pad_index(t)] = (t < HL_P && tg < L) ? kr[tg] : 0.f;
        im[pad_index(t)] = 0.f;
    }
    __syncthreads();
    hyena_train_fft<HL_LOGN, false>(re, im, tid, tw);
    const float inv = 1.0f / (float)HL_N;
    float2* out = kf + ((size_t)ch * S + j) * HL_H;
    for (int m = tid; m < HL_H; m += HL_NT)
        out[m] = make_float2(re[pad_index(m)] * inv, (m == 0 || m == HL_N / 2) ? 0.f : im[pad_index(m)] * inv);
}

// the bin pair (m, N - m) of the packed spectrum Z in LDS -> A2 = 2 A[m], B2 = 2 B[m] of its two real sequences
__device__ __forceinline__ void hl_separate(const float* re, const float* im, int m, int& n, int& pm, int& pn, float2& a2, float2& b2) {
    n = (HL_N - m) & (HL_N - 1), pm = pad_index(m), pn = pad_index(n);
    const float2 zm = make_float2(re[pm], im[pm]), zn = make_float2(re[pn], im[pn]);
    a2 = make_float2(zm.x + zn.x, zm.y - zn.y);                           // Z[m] + conj Z[n]
    b2 = make_float2(zm.y + zn.y, zn.x - zm.x);                           // -i (Z[m] - conj Z[n])
}
// tid again, as a value the compiler cannot trace: the LDS addresses of a transform's passes depend on tid alone, and hoisted out of
// the segment loop they stay in registers through every pass of every segment (measured: scratch)
__device__ __forceinline__ int hl_fresh(int tid) {
    asm volatile("" : "+v"(tid));
    return tid;
}
__device__ __forceinline__ float2 hl_mac(float2 a, float2 b, float2 acc) {                  // acc + a b
    return make_float2(fmaf(a.x, b.x, fmaf(-a.y, b.y, acc.x)), fmaf(a.x, b.y, fmaf(a.y, b.x, acc.y)));
}
// The product spectra S1[m], S2[m] of a thread's pair wait in the pair's own slots: S1 at m, S2 at N - m.  Bins 0 and N / 2 are their
// own mirror; both products are real there (every factor is) and share the one slot as (re, im) = (S1, S2).
__device__ __forceinline__ void hl_park(float* re, float* im, int m, int n, int pm, int pn, float2 s1, float2 s2, float& n1, float& n2) {
    if (n != m) {
        re[pm] = s1.x, im[pm] = s1.y, re[pn] = s2.x, im[pn] = s2.y;
        n1 = fmaf(2.f, s1.x * s1.x + s1.y * s1.y, n1);
        n2 = fmaf(2.f, s2.x * s2.x + s2.y * s2.y, n2);
    } else {
        re[pm] = s1.x, im[pm] = s2.x;
        n1 = fmaf(s1.x, s1.x, n1);
        n2 = fmaf(s2.x, s2.x, n2);
    }
}
// W = S1 + i r S2 over the parked products, r = the balance of their two norms (by Parseval, those of the two results); -> r
__device__ __forceinline__ float hl_pack(float* re, float* im, float* red, int tid, float n1, float n2) {
    const float2 tot = hyena_train_block_sum2<HL_NT>(n1, n2, red, tid);
    const float r = hyena_train_balance(tot.x, tot.y);
#pragma unroll 1
    for (int m = tid; m <= HL_N / 2; m += HL_NT) {
        const int n = (HL_N - m) & (HL_N - 1), pm = pad_index(m), pn = pad_index(n);
        if (n != m) {
            const float2 s1 = make_float2(re[pm], im[pm]), s2 = make_float2(re[pn] * r, im[pn] * r);
            re[pm] = s1.x - s2.y;
            im[pm] = s1.y + s2.x;
            re[pn] = s1.x + s2.y;                 // W[N - m] = conj S1 + i conj S2
            im[pn] = s2.x - s1.y;
        } else {
            im[pm] *= r;
        }
    }
    return r;
}

// One workgroup = (channel pair, read), segments in ascending order.  xs: [B, 128, S, 2, H] complex, A_i and B_i of this pair.
__global__ __launch_bounds__(HL_NT) void hyena_longtrain_fwd_kernel(const float* __restrict__ zc, const float* __restrict__ sw,
                                                                    const float* __restrict__ sb, const float* __restrict__ Dk,
                                                                    const float2* __restrict__ kf, const float2* tw,
                                                                    float2* xs, float* __restrict__ c, float* __restrict__ y,
                                                                    int L, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(HL_N);
    float* red = im + padded_size(HL_N);
    const int tid0 = threadIdx.x, c0 = 2 * blockIdx.x, c1 = c0 + 1, b = blockIdx.y;
    const float* zb = zc + (size_t)b * D3 * L;
    float2* xw = xs + ((size_t)b * (D / 2) + blockIdx.x) * S * 2 * HL_H;
    const float2* k0 = kf + (size_t)c0 * S * HL_H;
    const float2* k1 = kf + (size_t)c1 * S * HL_H;
    HtShort s0, s1;
    s0.load(sw, sb, c0);
    s1.load(sw, sb, c1);
    const float d0 = Dk[c0], d1 = Dk[c1];
    float* cr0 = c + ((size_t)b * D + c0) * L;
    float* yr0 = y + ((size_t)b * D + c0) * L;

    for (int i = 0; i < S; ++i) {
        const int tid = hl_fresh(tid0);
        float e0 = 0.f, e1 = 0.f;
        for (int t = tid; t < HL_N; t += HL_NT) {                         // z = [g_{i-1} ; g_i] of c0 + i the same of c1
            const int tg = (i - 1) * HL_P + t;
            float g0 = 0.f, g1 = 0.f;
            if (tg >= 0 && tg < L) {
                HtTaps a, e;
                hyena_train_taps(zb, c0, tg, L, s0, a);
                hyena_train_taps(zb, c1, tg, L, s1, e);
                g0 = a.u[2] * a.u[1];
                g1 = e.u[2] * e.u[1];
            }
            re[pad_index(t)] = g0;
            im[pad_index(t)] = g1;
            e0 = fmaf(g0, g0, e0);
            e1 = fmaf(g1, g1, e1);
        }
        const float2 nin = hyena_train_block_sum2<HL_NT>(e0, e1, red, tid);
        const float rin = hyena_train_balance(nin.x, nin.y), rinv = 1.0f / rin;      // powers of two: exact
        hyena_train_scale_im<HL_LOGN>(im, tid, HL_N, rin);
        __syncthreads();
        hyena_train_fft<HL_LOGN, false>(re, im, tid, tw);
        float n1 = 0.f, n2 = 0.f;
#pragma unroll 1
        for (int m = tid; m <= HL_N / 2; m += HL_NT) {
            int n, pm, pn;
            float2 a2, b2;
            hl_separate(re, im, m, n, pm, pn, a2, b2);
            const float2 A = make_float2(0.5f * a2.x, 0.5f * a2.y), Bv = make_float2(0.5f * rinv * b2.x, 0.5f * rinv * b2.y);
            xw[(size_t)(2 * i) * HL_H + m] = A;
            xw[(size_t)(2 * i + 1) * HL_H + m] = Bv;
            float2 p1 = cmul(A, k0[m]), p2 = cmul(Bv, k1[m]);
            for (int j = 1; j <= i; ++j) {
                p1 = hl_mac(xw[(size_t)(2 * (i - j)) * HL_H + m], k0[(size_t)j * HL_H + m], p1);
                p2 = hl_mac(xw[(size_t)(2 * (i - j) + 1) * HL_H + m], k1[(size_t)j * HL_H + m], p2);
            }
            hl_park(re, im, m, n, pm, pn, p1, p2, n1, n2);
        }
        const float rout = hl_pack(re, im, red, tid, n1, n2);
        __syncthreads();
        hyena_train_fft<HL_LOGN, true>(re, im, tid, tw);                  // [P .. 2 P): c_i of c0 | rout c_i of c1, without the skip term
        const float unscale = 1.0f / rout;
        for (int a_ = tid; a_ < HL_P; a_ += HL_NT) {
            const int tg = i * HL_P + a_;
            if (tg < L) {
                HtTaps a, e;
                hyena_train_taps(zb, c0, tg, L, s0, a);
                hyena_train_taps(zb, c1, tg, L, s1, e);
                const float v0 = fmaf(d0, a.u[2] * a.u[1], re[pad_index(HL_P + a_)]);
                const float v1 = fmaf(d1, e.u[2] * e.u[1], im[pad_index(HL_P + a_)] * unscale);
                cr0[tg] = v0;
                cr0[(size_t)L + tg] = v1;
                yr0[tg] = v0 * a.u[0];
                yr0[(size_t)L + tg] = v1 * e.u[0];
            }
        }
        __syncthreads();                                                  // the planes are free for the next segment
    }
}

// One workgroup = (channel, read).  Phase A stores W_m and G_m of every segment; phase B walks the segments from the last to the
// first, so that the two du values the transposed 3-tap filter needs from the next segment are at hand.  xs: [B, 256, S, 2, H].
__global__ __launch_bounds__(HL_NT) void hyena_longtrain_bwd_kernel(const float* __restrict__ zc, const float* __restrict__ sw,
                                                                    const float* __restrict__ sb, const float* __restrict__ Dk,
                                                                    const float* __restrict__ c, const float* __restrict__ dy,
                                                                    const float2* __restrict__ kf, const float2* tw,
                                                                    float2* xs, float* __restrict__ dzc,
                                                                    float* __restrict__ dkp, float* __restrict__ part, int L, int S) {
    constexpr int NW = HL_NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* re = reinterpret_cast<float*>(smem);
    float* im = re + padded_size(HL_N);
    float* red = im + padded_size(HL_N);          // [NW][HT_PART]
    const int tid0 = threadIdx.x, ch = blockIdx.x, b = blockIdx.y;
    const float* zb = zc + (size_t)b * D3 * L;
    const float* cr = c + ((size_t)b * D + ch) * L;
    const float* dyr = dy + ((size_t)b * D + ch) * L;
    float2* xw = xs + ((size_t)b * D + ch) * S * 2 * HL_H;
    const float2* kc = kf + (size_t)ch * S * HL_H;
    HtShort s;
    s.load(sw, sb, ch);

    for (int m_ = 0; m_ < S; ++m_) {                                      // phase A: z = [dc_m ; dc_{m+1}] + i r [g_m ; 0]
        const int tid = hl_fresh(tid0);
        float nd = 0.f, ng = 0.f;
        for (int t = tid; t < HL_N; t += HL_NT) {
            const int tg = m_ * HL_P + t;
            float dc = 0.f, g = 0.f;
            if (tg < L) {
                HtTaps a;
                hyena_train_taps(zb, ch, tg, L, s, a);
                dc = dyr[tg] * a.u[0];
                if (t < HL_P) g = a.u[2] * a.u[1];
            }
            re[pad_index(t)] = dc;
            im[pad_index(t)] = g;
            nd = fmaf(dc, dc, nd);
            ng = fmaf(g, g, ng);
        }
        const float2 nin = hyena_train_block_sum2<HL_NT>(nd, ng, red, tid);
        const float rin = hyena_train_balance(nin.x, nin.y), rinv = 1.0f / rin;
        hyena_train_scale_im<HL_LOGN>(im, tid, HL_P, rin);
        __syncthreads();
        hyena_train_fft<HL_LOGN, false>(re, im, tid, tw);
#pragma unroll 1
        for (int m = tid; m <= HL_N / 2; m += HL_NT) {
            int n, pm, pn;
            float2 a2, b2;
            hl_separate(re, im, m, n, pm, pn, a2, b2);
            xw[(size_t)(2 * m_) * HL_H + m] = make_float2(0.5f * a2.x, 0.5f * a2.y);
            xw[(size_t)(2 * m_ + 1) * HL_H + m] = make_float2(0.5f * rinv * b2.x, 0.5f * rinv * b2.y);
        }
        __syncthreads();
    }

    const float dskip = Dk[ch], invn = 1.0f / (float)HL_N;
    float acc[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) acc[j] = 0.f;
    float nx1[2] = {0.f, 0.f}, nv[2] = {0.f, 0.f};                        // dx1, dv at the next segment's tokens 0 and 1 (thread 0's count)
    float* dkr = dkp + ((size_t)b * D + ch) * L;
    float* dz0 = dzc + ((size_t)b * D3 + ch) * L;
    for (int i = S - 1; i >= 0; --i) {                                    // phase B
        const int tid = hl_fresh(tid0);
        float n1 = 0.f, n2 = 0.f;
#pragma unroll 1
        for (int m = tid; m <= HL_N / 2; m += HL_NT) {
            const int n = (HL_N - m) & (HL_N - 1), pm = pad_index(m), pn = pad_index(n);
            float2 p1 = make_float2(0.f, 0.f), p2 = make_float2(0.f, 0.f);
            for (int j = 0; j < S - i; ++j) {
                const float2 W = xw[(size_t)(2 * (i + j)) * HL_H + m];
                p1 = hl_mac(W, cconj(kc[(size_t)j * HL_H + m]), p1);
                p2 = hl_mac(W, cconj(xw[(size_t)(2 * j + 1) * HL_H + m]), p2);
            }
            p2.x *= invn, p2.y *= invn;
            hl_park(re, im, m, n, pm, pn, p1, p2, n1, n2);
        }
        const float rout = hl_pack(re, im, red, tid, n1, n2);
        __syncthreads();
        hyena_train_fft<HL_LOGN, true>(re, im, tid, tw);                  // [0 .. P): dg_i without the skip term | rout dk_i of this read
        const float unscale = 1.0f / rout;
        for (int t = tid; t < HL_P; t += HL_NT) {                         // planes become dx1 | dv of the segment
            const int tg = i * HL_P + t;
            float dx1 = 0.f, dv = 0.f;
            if (tg < L) {
                HtTaps a;
                hyena_train_taps(zb, ch, tg, L, s, a);
                const float dyt = dyr[tg], dc = dyt * a.u[0], g = a.u[2] * a.u[1], dx0 = dyt * cr[tg];
                dkr[tg] = im[pad_index(t)] * unscale;
                const float dg = fmaf(dskip, dc, re[pad_index(t)]);
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
            re[pad_index(t)] = dx1;
            im[pad_index(t)] = dv;
        }
        if (tid == 0) {                                                   // slots P and P + 1: the next segment's first two
            re[pad_index(HL_P)] = nx1[0], re[pad_index(HL_P + 1)] = nx1[1];
            im[pad_index(HL_P)] = nv[0], im[pad_index(HL_P + 1)] = nv[1];
        }
        __syncthreads();
        for (int t = tid; t < HL_P; t += HL_NT) {     // dzc[r, t] = sw[r, 2] du[t] + sw[r, 1] du[t + 1] + sw[r, 0] du[t + 2]
            const int tg = i * HL_P + t;
            if (tg < L) {
                float dx0[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) dx0[e] = tg + e < L ? dyr[tg + e] * cr[tg + e] : 0.f;
                const float* planes[2] = {re, im};
                dz0[tg] = fmaf(s.w[0][0], dx0[2], fmaf(s.w[0][1], dx0[1], s.w[0][2] * dx0[0]));
#pragma unroll
                for (int q = 1; q < 3; ++q) {
                    const float* p = planes[q - 1];
                    dz0[(size_t)q * D * L + tg] =
                        fmaf(s.w[q][0], p[pad_index(t + 2)], fmaf(s.w[q][1], p[pad_index(t + 1)], s.w[q][2] * p[pad_index(t)]));
                }
            }
        }
        if (tid == 0) {
            nx1[0] = re[pad_index(0)], nx1[1] = re[pad_index(1)];
            nv[0] = im[pad_index(0)], nv[1] = im[pad_index(1)];
        }
        __syncthreads();
    }
    // the row's partials: lanes in wave_sum's order, then waves in wave order
    const int tid = tid0;
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
__global__ __launch_bounds__(256) void hyena_longtrain_reduce_kernel(const float* __restrict__ dkp, const float* __restrict__ part,
                                                                     float* __restrict__ dk, float* __restrict__ dsw,
                                                                     float* __restrict__ dsb, float* __restrict__ dD, int B, int L) {
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

constexpr size_t HL_LDS = (size_t)(2 * padded_size(HL_N) + (HL_NT / 64) * HT_PART) * sizeof(float);       // 147,968 B

void hl_prepare(const float* k, float* ws, const HlLayout& lay, int L, int S, hipStream_t st) {
    float2* tw = reinterpret_cast<float2*>(ws + lay.tw);
    hipLaunchKernelGGL(hyena_longtrain_twiddle_kernel, dim3((HL_N / 2 + 255) / 256), dim3(256), 0, st, tw);
    launch_lds<hyena_longtrain_spectrum_kernel>(dim3(D, S), dim3(HL_NT), HL_LDS, st, k, reinterpret_cast<float2*>(ws + lay.kf),
                                                (const float2*)tw, L, S);
}

// CLM_OK, or why the shape is refused
int hl_shape(int B, int L) {
    if (B < 1 || L < 1 || B > 65535) return CLM_E_INVALID;
    return L > HL_MAX_TOKENS ? CLM_E_UNSUPPORTED : CLM_OK;
}
bool hl_ptrs(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p || (reinterpret_cast<uintptr_t>(p) & 3)) return false;
    return true;
}

}  // namespace

}  // namespace clm

using namespace clm;

extern "C" int64_t clm_hyena_longtrain_workspace_bytes(int B, int L) {
    const int rc = hl_shape(B, L);
    if (rc != CLM_OK) return rc;
    return ((int64_t)HlLayout(B, L).total * (int64_t)sizeof(float) + 15) & ~(int64_t)15;
}

extern "C" int clm_hyena_longtrain_forward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk, int B, int L,
                                           float* c_out, float* y_out, void* workspace, void* stream) {
    const int rc = hl_shape(B, L);
    if (rc != CLM_OK) return rc;
    if (!hl_ptrs({zc, sw, sb, k, Dk, c_out, y_out, workspace})) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const HlLayout lay(B, L);
    const int S = hl_segments(L);
    hl_prepare(k, ws, lay, L, S, st);
    launch_lds<hyena_longtrain_fwd_kernel>(dim3(D / 2, B), dim3(HL_NT), HL_LDS, st, zc, sw, sb, Dk,
                                           (const float2*)reinterpret_cast<float2*>(ws + lay.kf),
                                           (const float2*)reinterpret_cast<float2*>(ws + lay.tw), reinterpret_cast<float2*>(ws + lay.spec),
                                           c_out, y_out, L, S);
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}

extern "C" int clm_hyena_longtrain_backward(const float* zc, const float* sw, const float* sb, const float* k, const float* Dk,
                                            const float* c, const float* dy, int B, int L, float* dzc, float* dsw, float* dsb, float* dk,
                                            float* dD, void* workspace, void* stream) {
    const int rc = hl_shape(B, L);
    if (rc != CLM_OK) return rc;
    if (!hl_ptrs({zc, sw, sb, k, Dk, c, dy, dzc, dsw, dsb, dk, dD, workspace})) return CLM_E_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const HlLayout lay(B, L);
    const int S = hl_segments(L);
    hl_prepare(k, ws, lay, L, S, st);
    launch_lds<hyena_longtrain_bwd_kernel>(dim3(D, B), dim3(HL_NT), HL_LDS, st, zc, sw, sb, Dk, c, dy,
                                           (const float2*)reinterpret_cast<float2*>(ws + lay.kf),
                                           (const float2*)reinterpret_cast<float2*>(ws + lay.tw), reinterpret_cast<float2*>(ws + lay.spec),
                                           dzc, ws + lay.dkp, ws + lay.part, L, S);
    hipLaunchKernelGGL(hyena_longtrain_reduce_kernel, dim3((L + 255) / 256, D), dim3(256), 0, st, (const float*)(ws + lay.dkp),
                       (const float*)(ws + lay.part), dk, dsw, dsb, dD, B, L);
    return hipGetLastError() == hipSuccess ? CLM_OK : CLM_E_HIP;
}
