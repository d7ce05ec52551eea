// longread_plan.cpp -- the host side of `predict --long-reads tile`: token counts of a left-padded batch and the window plan.
// Plain C++, no HIP: it is part of the engine library and also compiles into a stand-alone program (tests/sanitize/longread_host.cpp).
//
// The reference truncates a read to the tokenizer's length (/root/reference/chimeralm/data/bam.py:166-170) and never sees the rest.
// The plan cuts a read of n bases into windows of exactly Wb bases that overlap by O (the last one right-aligned on the read's last
// base) and describes every row of the forwards as a span: which bytes of which source row it copies, and whether [SEP] follows.
// The definitions are in include/chimeralm_hip.h.
#include "longread_plan.h"

#include <climits>
#include <cstdint>

namespace clm {
namespace longread {

std::string& host_error() {
    static std::string s;
    return s;
}

namespace {
int refuse(const std::string& msg) {
    host_error() = msg;
    return CLM_E_INVALID;
}
}  // namespace

}  // namespace longread
}  // namespace clm

using namespace clm::longread;

extern "C" {

int clm_longread_lengths(const unsigned char* ids, int64_t row_stride, int B, int L, int32_t* n_tokens) {
    if (!ids || !n_tokens || B < 1 || L < 1 || row_stride < L) return refuse("clm_longread_lengths: bad argument");
    for (int r = 0; r < B; ++r) {
        const unsigned char* row = ids + (size_t)r * (size_t)row_stride;
        if (row[L - 1] == PAD_ID)
            return refuse("clm_longread_lengths: row " + std::to_string(r) + " ends in [PAD]: it is empty or not padded on the left");
        // the first column that is not [PAD]: columns below `lo` are pads, column `hi` is a token (L - 1 is one)
        int lo = 0, hi = L - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (row[mid] == PAD_ID) lo = mid + 1; else hi = mid;
        }
        if (row[lo] == PAD_ID || (lo > 0 && row[lo - 1] != PAD_ID))
            return refuse("clm_longread_lengths: row " + std::to_string(r) + " is not pads followed by tokens");
        n_tokens[r] = L - lo;
    }
    return CLM_OK;
}

int clm_longread_plan(const int32_t* n_tokens, int B, int L, int window, int overlap, int max_bases, int* L_out, int32_t* first,
                      clm_longread_span* spans, int32_t* starts, int capacity, int* n_spans) {
    if (!n_tokens || !L_out || !n_spans || B < 1 || L < 1) return refuse("clm_longread_plan: bad argument");
    if (window < 1 || window > INT_MAX - 16)
        return refuse("clm_longread_plan: the window has at least 1 base, got " + std::to_string(window));
    if (overlap < 0 || 2 * (int64_t)overlap > window)
        return refuse("clm_longread_plan: 0 <= overlap <= window / 2, got overlap " + std::to_string(overlap) + ", window " +
                      std::to_string(window));
    if (max_bases < window)
        return refuse("clm_longread_plan: max_bases >= window, got max_bases " + std::to_string(max_bases) + ", window " +
                      std::to_string(window));
    if (spans && capacity < 0) return refuse("clm_longread_plan: bad capacity");
    const int C = window + 1, step = window - overlap;              // (step >= ceil(window / 2) >= 1)
    const int width = L < C ? L : C;
    int64_t n_extra = 0;
    for (int r = 0; r < B; ++r) {
        if (n_tokens[r] < 1 || n_tokens[r] > L)
            return refuse("clm_longread_plan: row " + std::to_string(r) + " has " + std::to_string(n_tokens[r]) + " tokens of " +
                          std::to_string(L));
        const int nb = n_tokens[r] - 1;                             // bases; the last token is [SEP]
        const int n = nb < max_bases ? nb : max_bases;
        if (first) first[r] = (int32_t)n_extra;
        if (nb > window) n_extra += ((int64_t)n - window + step - 1) / step;
        if (n_extra > INT_MAX - B) return refuse("clm_longread_plan: too many windows");
    }
    if (first) first[B] = (int32_t)n_extra;
    *L_out = width;
    *n_spans = B + (int)n_extra;
    if (!spans) return CLM_OK;
    if (*n_spans > capacity)
        return refuse("clm_longread_plan: the plan has " + std::to_string(*n_spans) + " rows, capacity " + std::to_string(capacity));
    int e = B;
    for (int r = 0; r < B; ++r) {
        const int nb = n_tokens[r] - 1, col0 = L - n_tokens[r];
        if (nb <= window) {                                         // the read itself, its own [SEP] included
            spans[r] = clm_longread_span{r, col0, n_tokens[r], 0};
            if (starts) starts[r] = 0;
            continue;
        }
        const int n = nb < max_bases ? nb : max_bases;
        const int K = 1 + (int)(((int64_t)n - window + step - 1) / step);
        spans[r] = clm_longread_span{r, col0, window, CLM_LONGREAD_SEP};
        if (starts) starts[r] = 0;
        for (int k = 1; k < K; ++k, ++e) {
            const int64_t at = k < K - 1 ? (int64_t)k * step : (int64_t)n - window;
            spans[e] = clm_longread_span{r, col0 + (int)at, window, CLM_LONGREAD_SEP};
            if (starts) starts[e] = (int32_t)at;
        }
    }
    return CLM_OK;
}

}  // extern "C"
