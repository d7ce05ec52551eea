// bucket_plan.cpp -- the host side of `predict --batching bucket`: a read's canonical length and the regrouping plan.
// Plain C++, no HIP: it is part of the engine library and also compiles into a stand-alone program (tests/sanitize/bucket_host.cpp).
//
// The reference pads a batch on the left to its longest read (/root/reference/chimeralm/data/tokenizer.py:152-159), so a read's row
// -- and with it its logits -- depends on its batch-mates.  Here every read is padded to a length that depends on its own token count
// alone, and reads of one such length are forwarded together.  The planner takes the token counts of the incoming batches and says
// which bytes go where in a pool of per-class slabs (scatter steps) and when a class is forwarded (emit steps).  The definitions are
// in include/chimeralm_hip.h.
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "chimeralm_hip.h"

namespace {

std::string& host_error() {
    static std::string s;
    return s;
}

int64_t round16(int64_t n) { return (n + 15) / 16 * 16; }

bool good_steps(int steps_log2) { return steps_log2 >= 0 && steps_log2 <= 5; }

// Lc(n) of the header; n in 1 ... 32769, steps_log2 in 0 ... 5
int canonical(int n, int steps_log2) {
    const int b = n - 1;
    int lg = 0;
    while ((2 << lg) <= b) ++lg;                                   // floor(log2(max(b, 1)))
    const int e = lg - steps_log2 > 6 ? lg - steps_log2 : 6;
    const int q = 1 << e;
    const int k = b > 0 ? (b + q - 1) / q : 1;
    const int lc = 1 + q * k;
    return lc < CLM_BUCKET_MAX_TOKENS ? lc : CLM_BUCKET_MAX_TOKENS;
}

struct Class {
    int64_t offset = 0, stride = 0;
    std::vector<int64_t> reads;                                    // global indices of the rows it holds, in arrival order
};

}  // namespace

struct clm_bucket_plan {
    int batch_size = 0, steps_log2 = 0;
    int64_t pool_used = 0, n_pushed = 0;
    std::map<int, Class> classes;                                  // by Lc: `finish` walks them in ascending order
    std::vector<clm_bucket_step> steps;
    std::vector<clm_bucket_span> spans;
    std::vector<int64_t> reads;
    std::string err;

    int refuse(const std::string& msg) {
        err = msg;
        return CLM_E_INVALID;
    }
    void emit(int lc, Class& c) {
        steps.push_back(clm_bucket_step{CLM_BUCKET_EMIT, (int32_t)reads.size(), (int32_t)c.reads.size(), lc, c.offset, c.stride});
        reads.insert(reads.end(), c.reads.begin(), c.reads.end());
        c.reads.clear();
    }
};

extern "C" {

int clm_bucket_length(int n_tokens, int steps_log2) {
    if (n_tokens < 1 || n_tokens > CLM_BUCKET_MAX_TOKENS || !good_steps(steps_log2)) {
        host_error() = "clm_bucket_length: 1 <= n_tokens <= 32769 and 0 <= steps_log2 <= 5, got " + std::to_string(n_tokens) + ", " +
                       std::to_string(steps_log2);
        return CLM_E_INVALID;
    }
    return canonical(n_tokens, steps_log2);
}

int64_t clm_bucket_pool_bytes(int batch_size, int steps_log2) {
    if (batch_size < 1 || batch_size > 65535 || !good_steps(steps_log2)) {
        host_error() = "clm_bucket_pool_bytes: 1 <= batch_size <= 65535 and 0 <= steps_log2 <= 5";
        return CLM_E_INVALID;
    }
    int64_t row_bytes = 0;
    for (int n = 1; n <= CLM_BUCKET_MAX_TOKENS;) {                 // every class once: from a class top to the next class's first n
        const int lc = canonical(n, steps_log2);
        row_bytes += round16(lc);
        n = lc + 1;
    }
    return row_bytes * batch_size;
}

int clm_bucket_plan_create(int batch_size, int steps_log2, clm_bucket_plan** out) {
    if (!out || batch_size < 1 || batch_size > 65535 || !good_steps(steps_log2)) {
        host_error() = "clm_bucket_plan_create: 1 <= batch_size <= 65535 and 0 <= steps_log2 <= 5, got " + std::to_string(batch_size) +
                       ", " + std::to_string(steps_log2);
        return CLM_E_INVALID;
    }
    clm_bucket_plan* p = new clm_bucket_plan();
    p->batch_size = batch_size;
    p->steps_log2 = steps_log2;
    *out = p;
    return CLM_OK;
}

int clm_bucket_plan_push(clm_bucket_plan* p, const int32_t* n_tokens, int B, int L) {
    if (!p) return CLM_E_INVALID;
    if (!n_tokens || B < 1 || L < 1) return p->refuse("clm_bucket_plan_push: bad argument");
    for (int r = 0; r < B; ++r)                                    // all rows are checked before anything changes
        if (n_tokens[r] < 1 || n_tokens[r] > L || n_tokens[r] > CLM_BUCKET_MAX_TOKENS)
            return p->refuse("clm_bucket_plan_push: row " + std::to_string(r) + " has " + std::to_string(n_tokens[r]) + " tokens of " +
                             std::to_string(L) + " (1 ... 32769)");
    p->steps.clear();
    p->spans.clear();
    p->reads.clear();
    size_t group = 0;                                              // the first span of the open scatter group
    for (int r = 0; r < B; ++r) {
        const int n = n_tokens[r], lc = canonical(n, p->steps_log2);
        auto it = p->classes.find(lc);
        if (it == p->classes.end()) {                              // first use: the class's slab goes behind the pool's last
            Class c;
            c.offset = p->pool_used;
            c.stride = round16(lc);
            p->pool_used += c.stride * p->batch_size;
            it = p->classes.emplace(lc, std::move(c)).first;
        }
        Class& c = it->second;
        p->spans.push_back(clm_bucket_span{r, L - n, n, lc, c.offset + (int64_t)c.reads.size() * c.stride});
        c.reads.push_back(p->n_pushed++);
        if ((int)c.reads.size() == p->batch_size) {                // full: its rows are written, then forwarded, before the slab is reused
            p->steps.push_back(clm_bucket_step{CLM_BUCKET_SCATTER, (int32_t)group, (int32_t)(p->spans.size() - group), 0, 0, 0});
            p->emit(lc, c);
            group = p->spans.size();
        }
    }
    if (p->spans.size() > group)
        p->steps.push_back(clm_bucket_step{CLM_BUCKET_SCATTER, (int32_t)group, (int32_t)(p->spans.size() - group), 0, 0, 0});
    return CLM_OK;
}

int clm_bucket_plan_finish(clm_bucket_plan* p) {
    if (!p) return CLM_E_INVALID;
    p->steps.clear();
    p->spans.clear();
    p->reads.clear();
    for (auto& kv : p->classes)
        if (!kv.second.reads.empty()) p->emit(kv.first, kv.second);
    return CLM_OK;
}

int clm_bucket_plan_steps(const clm_bucket_plan* p, const clm_bucket_step** steps, int* n_steps, const clm_bucket_span** spans,
                          int* n_spans, const int64_t** reads, int* n_reads) {
    if (!p || !steps || !n_steps || !spans || !n_spans || !reads || !n_reads) return CLM_E_INVALID;
    *steps = p->steps.data();
    *n_steps = (int)p->steps.size();
    *spans = p->spans.data();
    *n_spans = (int)p->spans.size();
    *reads = p->reads.data();
    *n_reads = (int)p->reads.size();
    return CLM_OK;
}

const char* clm_bucket_plan_last_error(const clm_bucket_plan* p) { return p ? p->err.c_str() : host_error().c_str(); }

int clm_bucket_plan_destroy(clm_bucket_plan* p) {
    delete p;
    return CLM_OK;
}

}  // extern "C"
