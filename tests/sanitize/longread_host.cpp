// Stand-alone driver of csrc/longread_plan.cpp (plain C++, no HIP) for AddressSanitizer + UndefinedBehaviorSanitizer: the plan grid
// of tests/test_longread_host.py with buffers of exactly the size the count-only call reports, and the `lengths` cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "longread_plan.h"

#define REQUIRE(cond)                                                         \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int plan_case(int wb, int overlap, int n, int max_bases) {
    const int step = wb - overlap;
    // a batch of three rows: the read under test between a one-base read and a read of exactly the window
    const std::vector<int32_t> n_tokens = {2, n + 1, wb + 1};
    const int B = 3;
    int L = 2;
    for (int t : n_tokens) L = t > L ? t : L;
    int L_out = 0, n_spans = 0;
    std::vector<int32_t> first(B + 1, -1);
    REQUIRE(clm_longread_plan(n_tokens.data(), B, L, wb, overlap, max_bases, &L_out, first.data(), nullptr, nullptr, 0, &n_spans) == CLM_OK);
    REQUIRE(L_out == (L < wb + 1 ? L : wb + 1) && n_spans == B + first[B]);
    std::vector<clm_longread_span> spans((size_t)n_spans);
    std::vector<int32_t> starts((size_t)n_spans);
    if (n_spans > 1) {                                       // one short of what is needed: refused, the count still written
        int count = 0;
        REQUIRE(clm_longread_plan(n_tokens.data(), B, L, wb, overlap, max_bases, &L_out, first.data(), spans.data(), starts.data(),
                                  n_spans - 1, &count) == CLM_E_INVALID);
        REQUIRE(count == n_spans && clm::longread::host_error().size() > 0);
    }
    REQUIRE(clm_longread_plan(n_tokens.data(), B, L, wb, overlap, max_bases, &L_out, first.data(), spans.data(), starts.data(), n_spans,
                              &n_spans) == CLM_OK);
    const int m = n < max_bases ? n : max_bases;
    const int K = 1 + first[2] - first[1];
    REQUIRE(first[0] == 0 && first[1] == 0 && first[3] == first[2]);
    REQUIRE(K == (n <= wb ? 1 : 1 + (m - wb + step - 1) / step));
    std::vector<char> covered((size_t)(m > 0 ? m : 1), 0);
    int prev = 0;
    for (int k = 0; k < K; ++k) {
        const int row = k == 0 ? 1 : B + first[1] + k - 1;
        const clm_longread_span s = spans[(size_t)row];
        const int at = starts[(size_t)row];
        REQUIRE(s.read == 1 && s.src_col == L - n_tokens[1] + at);
        if (n <= wb) {
            REQUIRE(s.n_copy == n + 1 && s.flags == 0 && at == 0);
        } else {
            REQUIRE(s.n_copy == wb && s.flags == CLM_LONGREAD_SEP && at >= 0 && at + wb <= m);
            REQUIRE(k == 0 ? at == 0 : (at > prev && at - prev <= step));
            if (k == K - 1) REQUIRE(at + wb == m);
            for (int b = at; b < at + wb; ++b) covered[(size_t)b] = 1;
        }
        REQUIRE(s.src_col >= 0 && s.src_col + s.n_copy <= L);
        prev = at;
    }
    if (n > wb)
        for (int b = 0; b < m; ++b) REQUIRE(covered[(size_t)b]);
    return 0;
}

static int lengths_cases() {
    const int L = 37, B = 6;
    const int want[B] = {37, 1, 2, 20, 36, 19};
    std::vector<unsigned char> ids((size_t)B * L, 4);
    for (int r = 0; r < B; ++r) {
        for (int c = L - want[r]; c < L - 1; ++c) ids[(size_t)r * L + c] = (unsigned char)(7 + (c % 4));
        ids[(size_t)r * L + L - 1] = 1;
    }
    std::vector<int32_t> got((size_t)B, -1);
    REQUIRE(clm_longread_lengths(ids.data(), L, B, L, got.data()) == CLM_OK);
    for (int r = 0; r < B; ++r) REQUIRE(got[(size_t)r] == want[r]);
    std::vector<unsigned char> row((size_t)L, 4);                     // pads only
    REQUIRE(clm_longread_lengths(row.data(), L, 1, L, got.data()) == CLM_E_INVALID);
    for (int c = 0; c < 10; ++c) row[(size_t)c] = 7;                  // padded on the right
    REQUIRE(clm_longread_lengths(row.data(), L, 1, L, got.data()) == CLM_E_INVALID);
    REQUIRE(clm_longread_lengths(nullptr, L, 1, L, got.data()) == CLM_E_INVALID);
    REQUIRE(clm_longread_lengths(row.data(), L - 1, 1, L, got.data()) == CLM_E_INVALID);
    return 0;
}

int main() {
    const int wbs[] = {1, 2, 15, 16, 17, 64};
    int cases = 0;
    for (int wb : wbs) {
        const int overlaps[] = {0, 1, wb / 2};
        for (int overlap : overlaps) {
            if (2 * overlap > wb) continue;
            const int step = wb - overlap;
            const int ns[] = {0, 1, wb - 1, wb, wb + 1, wb + step - 1, wb + step, wb + step + 1, 5 * wb + 3};
            for (int n : ns)
                for (int max_bases : {5 * wb + 3, 2 * wb + 1}) {
                    if (plan_case(wb, overlap, n, max_bases)) return 1;
                    ++cases;
                }
        }
    }
    int L_out = 0, n_spans = 0;
    const int32_t one[1] = {5};
    if (clm_longread_plan(one, 1, 8, 4, 3, 16, &L_out, nullptr, nullptr, nullptr, 0, &n_spans) != CLM_E_INVALID ||   // overlap > window / 2
        clm_longread_plan(one, 1, 8, 0, 0, 16, &L_out, nullptr, nullptr, nullptr, 0, &n_spans) != CLM_E_INVALID ||   // window < 1
        clm_longread_plan(one, 1, 8, 4, 2, 3, &L_out, nullptr, nullptr, nullptr, 0, &n_spans) != CLM_E_INVALID ||    // max_bases < window
        clm_longread_plan(one, 1, 4, 4, 2, 16, &L_out, nullptr, nullptr, nullptr, 0, &n_spans) != CLM_E_INVALID) {   // more tokens than L
        std::fprintf(stderr, "a bad option was not refused\n");
        return 1;
    }
    if (lengths_cases()) return 1;
    std::printf("longread host driver OK: %d plan cases\n", cases);
    return 0;
}
