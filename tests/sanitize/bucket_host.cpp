// Stand-alone driver of csrc/bucket_plan.cpp (plain C++, no HIP) for AddressSanitizer + UndefinedBehaviorSanitizer: the grid of
// tests/test_bucket_host.py -- 2,000 seeded reads and every ladder edge, pushed in batches of 1, 7 and 64 at batch sizes 1, 3 and
// 256 -- with the plan's invariants checked from the definitions in include/chimeralm_hip.h.
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#include "chimeralm_hip.h"

#define REQUIRE(cond)                                                         \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static int64_t round16(int64_t n) { return (n + 15) / 16 * 16; }

static std::vector<int32_t> make_reads(int steps_log2) {
    std::vector<int32_t> n;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 2000; ++i) {                                 // roughly log-uniform in 1 ... 32769: a random octave, then a random offset
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int oct = (int)((s >> 33) % 16);
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int64_t v = ((int64_t)1 << oct) + (int64_t)((s >> 33) % ((uint64_t)1 << oct));
        n.push_back((int32_t)(v > CLM_BUCKET_MAX_TOKENS ? CLM_BUCKET_MAX_TOKENS : v));
    }
    for (int t = 1; t <= CLM_BUCKET_MAX_TOKENS;) {                   // every class top and its two neighbours
        const int lc = clm_bucket_length(t, steps_log2);
        for (int d = -1; d <= 1; ++d)
            if (lc + d >= 1 && lc + d <= CLM_BUCKET_MAX_TOKENS) n.push_back(lc + d);
        t = lc + 1;
    }
    return n;
}

struct Seen {
    std::vector<char> emitted;
    std::map<int, std::vector<int64_t>> held;                        // Lc -> the reads its slab holds, in arrival order
    std::set<int64_t> live;                                          // pool offsets of the rows that are written and not yet emitted
    int64_t next = 0;
};

static int walk(clm_bucket_plan* p, const std::vector<int32_t>& all, const int32_t* n_tokens, int B, int L, int batch_size, int steps_log2,
                int64_t pool, bool finish, Seen& seen) {
    const clm_bucket_step* steps = nullptr;
    const clm_bucket_span* spans = nullptr;
    const int64_t* reads = nullptr;
    int n_steps = 0, n_spans = 0, n_reads = 0;
    REQUIRE(clm_bucket_plan_steps(p, &steps, &n_steps, &spans, &n_spans, &reads, &n_reads) == CLM_OK);
    REQUIRE(finish ? n_spans == 0 : n_spans == B);
    int at = 0, prev_kind = -1, prev_length = 0;
    for (int i = 0; i < n_steps; ++i) {
        const clm_bucket_step st = steps[i];
        if (st.kind == CLM_BUCKET_SCATTER) {
            REQUIRE(!finish && prev_kind != CLM_BUCKET_SCATTER && st.first == at && st.count >= 1 && st.first + st.count <= n_spans);
            for (int k = st.first; k < st.first + st.count; ++k) {
                const clm_bucket_span sp = spans[k];
                const int n = n_tokens[sp.src_row];
                REQUIRE(sp.src_row == k && sp.n_copy == n && sp.src_col == L - n && sp.dst_width == clm_bucket_length(n, steps_log2));
                REQUIRE(sp.dst_width >= n && sp.dst_width >= 65 && sp.dst_offset % 16 == 0 && sp.dst_offset >= 0);
                REQUIRE(sp.dst_offset + round16(sp.dst_width) <= pool);
                REQUIRE(seen.live.insert(sp.dst_offset).second);                 // no two live rows share pool bytes (rows of a slab
                seen.held[sp.dst_width].push_back(seen.next++);                  // are stride apart; slabs are checked at the emit)
            }
            at = st.first + st.count;
        } else {
            REQUIRE(st.kind == CLM_BUCKET_EMIT && st.count >= 1 && st.count <= batch_size && st.stride == round16(st.length));
            REQUIRE(finish ? st.length > prev_length : (st.count == batch_size && prev_kind == CLM_BUCKET_SCATTER));
            std::vector<int64_t>& held = seen.held[st.length];
            REQUIRE((int)held.size() == st.count && st.first + st.count <= n_reads);
            for (int k = 0; k < st.count; ++k) {
                const int64_t r = reads[st.first + k];
                REQUIRE(r == held[(size_t)k] && r >= 0 && r < (int64_t)seen.emitted.size() && !seen.emitted[(size_t)r]);
                REQUIRE(clm_bucket_length(all[(size_t)r], steps_log2) == st.length);
                REQUIRE(seen.live.erase(st.offset + k * st.stride) == 1);
                seen.emitted[(size_t)r] = 1;
            }
            held.clear();
            prev_length = st.length;
        }
        prev_kind = st.kind;
    }
    REQUIRE(finish || at == n_spans);
    return 0;
}

static int run(int batch_size, int push, int steps_log2) {
    const std::vector<int32_t> all = make_reads(steps_log2);
    const int64_t pool = clm_bucket_pool_bytes(batch_size, steps_log2);
    REQUIRE(pool > 0);
    clm_bucket_plan* p = nullptr;
    REQUIRE(clm_bucket_plan_create(batch_size, steps_log2, &p) == CLM_OK && p);
    Seen seen;
    seen.emitted.assign(all.size(), 0);
    for (size_t i = 0; i < all.size(); i += (size_t)push) {
        const int B = (int)(all.size() - i < (size_t)push ? all.size() - i : (size_t)push);
        int L = 0;
        for (int r = 0; r < B; ++r) L = all[i + (size_t)r] > L ? all[i + (size_t)r] : L;
        REQUIRE(clm_bucket_plan_push(p, all.data() + i, B, L) == CLM_OK);
        if (walk(p, all, all.data() + i, B, L, batch_size, steps_log2, pool, false, seen)) return 1;
        for (const auto& kv : seen.held) REQUIRE((int)kv.second.size() < batch_size);      // a class emits exactly when it is full
    }
    REQUIRE(clm_bucket_plan_finish(p) == CLM_OK);
    if (walk(p, all, nullptr, 0, 0, batch_size, steps_log2, pool, true, seen)) return 1;
    for (char e : seen.emitted) REQUIRE(e);
    REQUIRE(seen.live.empty());
    const int32_t bad[2] = {5, 9};                                   // a refused push changes nothing
    REQUIRE(clm_bucket_plan_push(p, bad, 2, 8) == CLM_E_INVALID && clm_bucket_plan_last_error(p)[0] != 0);
    REQUIRE(clm_bucket_plan_finish(p) == CLM_OK);
    int n_steps = -1, n_spans = -1, n_reads = -1;
    const clm_bucket_step* steps = nullptr;
    const clm_bucket_span* spans = nullptr;
    const int64_t* reads = nullptr;
    REQUIRE(clm_bucket_plan_steps(p, &steps, &n_steps, &spans, &n_spans, &reads, &n_reads) == CLM_OK && n_steps == 0 && n_reads == 0);
    REQUIRE(clm_bucket_plan_destroy(p) == CLM_OK);
    return 0;
}

int main() {
    int classes = 0;
    for (int t = 1; t <= CLM_BUCKET_MAX_TOKENS; ++classes) t = clm_bucket_length(t, 3) + 1;
    REQUIRE(classes == 56 && clm_bucket_pool_bytes(1, 3) == 406400);
    REQUIRE(clm_bucket_length(0, 3) == CLM_E_INVALID && clm_bucket_length(32770, 3) == CLM_E_INVALID);
    REQUIRE(clm_bucket_length(100, -1) == CLM_E_INVALID && clm_bucket_length(100, 6) == CLM_E_INVALID);
    REQUIRE(clm_bucket_plan_last_error(nullptr)[0] != 0);
    clm_bucket_plan* p = nullptr;
    REQUIRE(clm_bucket_plan_create(0, 3, &p) == CLM_E_INVALID && clm_bucket_plan_create(65536, 3, &p) == CLM_E_INVALID);
    REQUIRE(clm_bucket_plan_create(4, 6, &p) == CLM_E_INVALID && clm_bucket_plan_create(4, 3, nullptr) == CLM_E_INVALID && !p);
    REQUIRE(clm_bucket_pool_bytes(0, 3) == CLM_E_INVALID && clm_bucket_plan_push(nullptr, nullptr, 1, 1) == CLM_E_INVALID);
    int runs = 0;
    for (int batch_size : {1, 3, 256})
        for (int push : {1, 7, 64})
            for (int steps_log2 : {3, 0, 5}) {
                if (steps_log2 != 3 && push != 7) continue;
                if (run(batch_size, push, steps_log2)) return 1;
                ++runs;
            }
    std::printf("bucket host driver OK: %d runs\n", runs);
    return 0;
}
