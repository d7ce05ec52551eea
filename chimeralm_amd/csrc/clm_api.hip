// clm_api.hip -- C ABI (include/chimeralm_hip.h) and host-side orchestration of the forward pass.
// The call sequence mirrors the reference protocol HyenaDna.forward -> backbone -> head
// (/root/reference/chimeralm/models/components/hyena.py:244-256); the operator order inside is the
// HyenaDNA block order of SURVEY.md section 8(a) rows 5-13.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <algorithm>
#include <string>
#include <vector>

#include "chimeralm_hip.h"
#include "handle_host.h"

using namespace clm;

namespace clm {
// "name" present in the comma-separated CLM_DEBUG list?  Read from the environment at every call (handles created one after the other
// in one process may differ); the per-launch users cache their answer.
bool debug_flag(const char* name) {
    const char* e = std::getenv("CLM_DEBUG");
    if (!e) return false;
    const size_t n = std::strlen(name);
    for (const char* p = e; *p;) {
        const char* q = std::strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : std::strlen(p);
        if (len == n && std::strncmp(p, name, n) == 0) return true;
        p += len + (q ? 1 : 0);
    }
    return false;
}
}  // namespace clm

namespace {

struct Tensor {
    DevBuf d;
    bool loaded = false;
};

// The filters of the four layers for one CLASS of lengths, built once and kept: the implicit filter's taps do not depend on L
// (k[t] is a function of t and the weights), and the spectrum of the first N/2 + 1 taps serves every L that runs through the
// N-point transform (L <= N/2 + 1: extra taps only reach outputs beyond L and nothing aliases, except the one product the
// convolution kernel already removes at L = N/2 + 1).  key = log2 N for single-shot lengths; KEY_LONG for L > 8193: the
// partition spectra K'_j of ALL taps (every long L uses a prefix of them).  Ragged real-world batches therefore never
// rebuild a filter (a rebuild per batch cost 3x at the reference's default batch of 12).
constexpr int KEY_LONG = 100;
struct ReversedFilter {           // conv_lone_tail(L): [256][stride] per layer, one per such L (16385, 24577, 32769)
    int L = 0, stride = 0;
    DevBuf p[NLAYER];
};
struct FilterSet {
    int key = 0, Lf = 0, logn = 0, KS = 1;   // Lf taps; KS partition spectra per channel in kf ([256][KS][N])
    DevBuf ktime[NLAYER], kf[NLAYER], tw;
    DevBuf kfp[NLAYER];           // 16384-point class only: kf lane-packed for the persistent kernel (launch_spectrum_lanepack)
    std::vector<ReversedFilter> krev;
};

// Weights as the kernels take them: device pointers resolved ONCE, by clm_finalize (a key that is not there fails there, with
// CLM_E_MISSING, instead of reaching a kernel as a null pointer).  The four products of a block are in_proj, out_proj, fc1, fc2,
// [MAT_N][MAT_K] each: the order of BlockF32::w and of a Packing's slots
constexpr int MAT_N[4] = {D3, D, DI, D}, MAT_K[4] = {D, D, D, DI};
struct BlockF32 {                 // one block's tensors as loaded, fp32
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const float* w[4];            // [out][in]: what the packers, the id table and the lone-token kernels read
    const float *b_in, *b_out, *b_fc1, *b_fc2;
    const float *short_w, *short_b;             // [768][3], [768]
    const float* filt_bias;                     // [256]  (D skip term)
    const float *pos_z, *pos_t, *f_w0, *f_b0, *f_freq, *f_w2, *f_b2, *f_w4, *f_b4, *f_w6, *deltas;   // the implicit filter (launch_filter)
};
struct NetF32 {                   // ... and what belongs to no block: embedding table, ln_f, the score layer, the classifier's matrices
    const float *emb, *lnf_g, *lnf_b, *att_w1, *att_b1, *att_w2, *att_b2, *cls[5];
};
// One packing of the matrices the MFMA kernels read: the four of every block and the score layer (attention.0.weight)
struct Packing {
    DevBuf w[NLAYER][4], score;
    DevBuf& slot(int i, int j) { return i < NLAYER ? w[i][j] : score; }   // i == NLAYER: the score layer
};
struct BlockW {                   // block i as one chunk's kernels read it (block_weights)
    const BlockF32* f;
    const void *w_in, *w_out, *w_fc1, *w_fc2;   // packed MFMA-fragment order, compute dtype: the GEMM kernels and the 16-bit tail
    const void *t_in, *t_out, *t_fc1, *t_fc2;   // exact fp32 / fp16x3: the fused tail's packing (tail32.hip)
};

}  // namespace

struct clm_handle {
    clm_config cfg{};
    int device = 0;
    std::string err;
    std::map<std::string, Tensor> w;
    bool finalized = false;
    // the weights resolved by clm_finalize (pointers into `w`) and their packings, one per kind (a chunk's choice: block_weights)
    BlockF32 blk[NLAYER] = {};
    NetF32 net = {};
    Packing pk_mode;              // cfg.precision (fp16c: fc1 / fc2 plain fp16 -- tail16_kernel, MLP_PREC)
    // 16-bit handles: exact-fp32 packing of the same weights for the GEMM kernels (fp16c's reads shorter than f16c_min_len,
    // clm_selfcheck, clm_set_fallback)
    Packing pk_f32;
    // exact fp32 (the engine's own mode, or the referee / short-read / fall-back path of a 16-bit engine): the fused tail's packing
    Packing pk_t32;               // (tail32.hip; its score layer: T32_SCORE)
    // the same weights as hi + lo halfs (launch_pack_x3; tail32.hip AR_X3): the arithmetic of a CLM_PREC_F16X3 handle AND, round 5,
    // of every 16-bit handle's short reads and first fall-back level
    Packing pk_x3;
    // PREC_F16C: fc1 / fc2 (slots 2, 3 alone) packed as hi + lo as well (the mode's second level, clm_set_mlp_compensation)
    Packing pk_mlpc;
    bool mlp_lo = false;
    int f16c_min_len = 2048;
    DevBuf sc_logits;             // [2][B][2] fp32: logits of the two passes of a self-check
    // host batches: two device staging buffers fed by the handle's own copy stream
    struct Stage {
        DevBuf buf;
        int dtype = 0, B = 0, L = 0;
        int64_t stride = 0;
        hipEvent_t copied = nullptr, consumed = nullptr;
        bool used = false, pending = false;
    } stage[2];
    hipStream_t copy_stream = nullptr;
    int next_stage = 0;
    int* bad_ids = nullptr;       // host-mapped flag the id kernels set for a token id outside [0, vocab_rows)
    DevBuf ztab;                  // [16][768] block-0 in_proj rows per token id (16-bit modes)
    // gated hand-over of z (TailArgs::zg): filter constants per layer, raw rows either side of the tail kernel's workgroup-range
    // boundaries, raw rows of every read's last two tiled tokens
    DevBuf fir[NLAYER];           // float4 [256][3]
    DevBuf edge_bnd, edge_read;   // float2
    bool raw_z = false;           // CLM_DEBUG=raw_z: the fused in_proj stage writes x0 | x1 | v as before round 3 (A/B runs, tests)
    bool row_h = false;           // CLM_DEBUG=row_h: the fused 16-bit tail kernels keep h in row order in every tile (A/B runs, tests)
    DevBuf head_t[5];
    HeadW hw{};
    std::vector<FilterSet> filters;
    // workspace (one chunk of reads; ensure_workspace)
    size_t ws_es = 0;             // element size z / y were last written with
    DevBuf h;                     // fp32 residual stream
    DevBuf z, y, u;
    DevBuf scores, stats, partial, pooled, lone_ws;   // fp32
    DevBuf gscratch;                                // float2: segment spectra of the long-read convolution
    DevBuf ylo;                                     // PREC_F16C: lo bytes of y [B][256][Lp] (round 4, clm_common.h lo8_pack4)
    DevBuf ids8;                                    // clamped ids [B][Lp]
    DevBuf traj_pooled, traj_npad;                  // the running verdict (trajectory.hip): fp32 [B][K][256], int [B]; grown by the first request
    // Round 5, the [PAD] prefix of left-padded batches (pad_prefix.hip): per read the 128-token tiles wholly inside its leading run
    // of [PAD], the list of tiles the tail kernels compute, and per arithmetic one table of what an all-[PAD] read leaves behind
    DevBuf pad_p0;                                  // int [3][B]: p0 | pair order | pair partner (launch_pair_order)
    DevBuf tile_list;                               // int [1 + B * tiles_x]
    struct PadTable {
        int prec = -1;                              // the arithmetic it was computed in (effective precision, fp16c's level, fp32 path: x3?)
        bool mlp_lo = false, x3 = false;
        int L = 0, Lp = 0;                          // tokens of the all-[PAD] read, row pitch of its z blocks
        DevBuf z[NLAYER];                           // [i], i >= 1: the z block layer i's convolution reads ([D3][Lp] elements incl. lo planes)
        DevBuf scores;                              // fp32 [L] pooling scores                              (16-bit fused path)
        DevBuf partial;                             // fp32 [ceil(L / 128)][POOL_PSTRIDE] pooling partials  (16-bit fused path)
        DevBuf hfin;                                // fp32 [L][256] the last block's residual rows         (fp32 path; its partials: per 64 tokens)
        // 16-bit fused path, tables of long reads (S = segments of L > 1): per block the segment spectra of the all-[PAD] read's
        // gated signal ([256][S][N], the one read's convolution scratch as it stood) and the running per-thread sums of the last
        // token's dot product -- segments inside the [PAD] prefix of both reads of a pair are not transformed (hyena_conv.hip SegPrefix)
        int S = 1;
        DevBuf gspec[NLAYER];                       // float2
        DevBuf dots[NLAYER];                        // fp32
    };
    std::vector<PadTable> pad_tables;
    DevBuf pad_ids;                                 // all PAD_ID: the table read's ids
    DevBuf pad_logits;                              // fp32 [2]: that read's logits (unused)
    bool no_pad_skip = false;                       // CLM_DEBUG=no_pad_skip: every tile of every read is computed (A/B runs, tests)
    bool no_seg_skip = false;                       // CLM_DEBUG=no_seg_skip: ... but every segment of the long-read convolution is transformed
    int last_B = 0, last_L = 0, last_Lp = 0;
    int last_hreg_Lmain = 0;      // > 0: the last chunk left the 128-token tiles of rows [0, Lmain) of h in register order (ChunkPlan::hreg)
    // The final residual rows as an output (clm_rows; the head fine-tune, pool_train.hip): what the last forward left in `h`, and a
    // counter that moves whenever anything may have rewritten that buffer (every chunk of every forward, a weight reload)
    struct RowsState {
        bool valid = false, one_chunk = false, exact = false;   // a forward completed / in ONE chunk / on the exact-fp32 or fp16x3 kernels
        int B = 0, L = 0;
        int64_t generation = 0;
    } rows;
    DevBuf pt_w1s, pt_w1t, pt_partial;    // clm_pool_forward / _backward: W1 packed for the score GEMM / the tiles, partials
    // How forwards run right now.  clm_selfcheck / clm_set_fallback: the exact-fp32 kernels of the same handle as referee of, and
    // replacement for, the 16-bit path; clm_selfcheck and the build of a [PAD] table change it for a scope (RunScope)
    struct RunMode {
        int force_prec = -1;      // >= 0 inside clm_selfcheck / a table build: the arithmetic forward_chunk runs in, whatever the length
        // clm_set_fallback: 0 = the handle's own mode; 1 = the next arithmetic INSIDE the gate (a 16-bit handle: fp16x3 -- fp32-class
        // results at about twice the exact rate; an fp16x3 handle: exact fp32); 2 = exact fp32 on every handle
        int fallback = 0;
        bool referee = false;     // inside clm_selfcheck's second pass: exact fp32, whatever the handle's mode or fall-back level
        bool prof = false;        // clm_profile_enable: StageTimer records its spans
        PadTable* capture = nullptr;   // inside the forward that fills a table
    } run;
    // debug / profiling
    int stop_layer = -1, stop_stage = -1;
    bool no_idconv = false;       // CLM_DEBUG=no_idconv: run block 0's in_proj instead of the id-table convolution (A/B runs)
    int conv_flags = 0;           // CLM_DEBUG=conv_oneshot / conv_no_xcd: CONV_* switches of the convolution launchers (A/B runs, tests)
    bool no_lone_peel = false;    // CLM_DEBUG=no_lone_peel: keep the lone last token of 128 k + 1-token reads in a tile of its own (A/B runs)
    bool x3 = false;              // CLM_PREC_F16X3: cfg.precision is PREC_F32 inside the engine, the fused tails run on hi + lo halfs (tail32.hip AR_X3)
    float x3_wmax = 0.f;          // largest |w| of the hi + lo packed weights (clm_finalize; NaN if any is NaN): from X3_WEIGHT_LIMIT on, exact fp32
    bool unfused_fp32 = false;    // CLM_DEBUG=unfused_fp32: exact fp32 through the separate GEMM kernels of rounds 1-3 (tests cross-check the fused tail)
    StageProfile<CLM_N_STAGES> profile;
};

namespace {

size_t elem_size(int prec) { return prec == PREC_F32 ? 4 : 2; }
int round_up(int v, int m) { return (v + m - 1) / m * m; }
int tiles_of(int L, int tile) { return (L + tile - 1) / tile; }
// Row pitch (tokens) of the channel-major planes z / y and their lo-byte planes.  (A multiple of the 128-token tile, so that a
// tile's piece of a BYTE row is one whole 128-byte line instead of straddling two on every other row, was measured in round 4:
// tail kernel 21.7 vs 21.5 ms per step on one box, three alternations -- not kept.)
constexpr int LP_ALIGN = 64;

// ---- expected weights: key, shape, and where clm_finalize puts the device pointer ---------------------
struct KeySpec {
    std::string key;
    std::vector<int64_t> shape;
    const float** dst;
};

std::vector<KeySpec> expected_keys(clm_handle* h) {
    std::vector<KeySpec> k;
    const clm_config& c = h->cfg;
    const int64_t d = c.d_model, di = c.d_inner, fo = c.filter_order, hh = c.head_hidden;
    NetF32& n = h->net;
    k.push_back({"bb.embeddings.word_embeddings.weight", {c.vocab_rows, d}, &n.emb});
    for (int i = 0; i < c.n_layer; ++i) {
        BlockF32& b = h->blk[i];
        std::string p = "bb.layers." + std::to_string(i) + ".";
        k.push_back({p + "norm1.weight", {d}, &b.ln1_g});
        k.push_back({p + "norm1.bias", {d}, &b.ln1_b});
        k.push_back({p + "norm2.weight", {d}, &b.ln2_g});
        k.push_back({p + "norm2.bias", {d}, &b.ln2_b});
        k.push_back({p + "mixer.in_proj.weight", {3 * d, d}, &b.w[0]});
        k.push_back({p + "mixer.in_proj.bias", {3 * d}, &b.b_in});
        k.push_back({p + "mixer.out_proj.weight", {d, d}, &b.w[1]});
        k.push_back({p + "mixer.out_proj.bias", {d}, &b.b_out});
        k.push_back({p + "mixer.short_filter.weight", {3 * d, 1, 3}, &b.short_w});
        k.push_back({p + "mixer.short_filter.bias", {3 * d}, &b.short_b});
        std::string f = p + "mixer.filter_fn.";
        k.push_back({f + "bias", {d}, &b.filt_bias});
        k.push_back({f + "pos_emb.z", {1, c.max_seq_len, c.emb_dim}, &b.pos_z});
        k.push_back({f + "pos_emb.t", {1, c.max_seq_len, 1}, &b.pos_t});
        k.push_back({f + "implicit_filter.0.weight", {fo, c.emb_dim}, &b.f_w0});
        k.push_back({f + "implicit_filter.0.bias", {fo}, &b.f_b0});
        k.push_back({f + "implicit_filter.1.freq", {1, fo}, &b.f_freq});
        k.push_back({f + "implicit_filter.2.weight", {fo, fo}, &b.f_w2});
        k.push_back({f + "implicit_filter.2.bias", {fo}, &b.f_b2});
        k.push_back({f + "implicit_filter.4.weight", {fo, fo}, &b.f_w4});
        k.push_back({f + "implicit_filter.4.bias", {fo}, &b.f_b4});
        k.push_back({f + "implicit_filter.6.weight", {d, fo}, &b.f_w6});
        k.push_back({f + "modulation.deltas", {1, 1, d}, &b.deltas});
        k.push_back({p + "mlp.fc1.weight", {di, d}, &b.w[2]});
        k.push_back({p + "mlp.fc1.bias", {di}, &b.b_fc1});
        k.push_back({p + "mlp.fc2.weight", {d, di}, &b.w[3]});
        k.push_back({p + "mlp.fc2.bias", {d}, &b.b_fc2});
    }
    k.push_back({"bb.ln_f.weight", {d}, &n.lnf_g});
    k.push_back({"bb.ln_f.bias", {d}, &n.lnf_b});
    k.push_back({"head.attention.0.weight", {hh / 2, d}, &n.att_w1});
    k.push_back({"head.attention.0.bias", {hh / 2}, &n.att_b1});
    k.push_back({"head.attention.2.weight", {1, hh / 2}, &n.att_w2});
    k.push_back({"head.attention.2.bias", {1}, &n.att_b2});
    k.push_back({"head.classifier.0.weight", {hh, d}, &n.cls[0]});
    k.push_back({"head.classifier.0.bias", {hh}, &h->hw.b0});
    k.push_back({"head.classifier.3.weight", {hh, hh}, &n.cls[1]});
    k.push_back({"head.classifier.3.bias", {hh}, &h->hw.b3});
    k.push_back({"head.classifier.6.layers.0.weight", {hh, hh}, &n.cls[2]});
    k.push_back({"head.classifier.6.layers.0.bias", {hh}, &h->hw.b60});
    k.push_back({"head.classifier.6.layers.3.weight", {hh, hh}, &n.cls[3]});
    k.push_back({"head.classifier.6.layers.3.bias", {hh}, &h->hw.b63});
    k.push_back({"head.output_layer.weight", {c.n_classes, hh}, &n.cls[4]});
    k.push_back({"head.output_layer.bias", {c.n_classes}, &h->hw.bo});
    return k;
}

// "net.backbone.backbone.X" | "backbone.backbone.X" | "backbone.X" -> "bb.X";  "net.head.Y" | "head.Y" -> "head.Y"
bool canonical_key(const char* key, std::string& out) {
    std::string s(key);
    if (s.rfind("net.", 0) == 0) s = s.substr(4);
    if (s.rfind("backbone.backbone.", 0) == 0) {
        out = "bb." + s.substr(18);
        return true;
    }
    if (s.rfind("backbone.", 0) == 0) {
        out = "bb." + s.substr(9);
        return true;
    }
    if (s.rfind("head.", 0) == 0) {
        out = s;
        return true;
    }
    return false;
}

__global__ void convert_to_f32_kernel(const void* in, float* out, size_t n, int dtype) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dtype == CLM_DT_F64)
        out[i] = (float)reinterpret_cast<const double*>(in)[i];
    else if (dtype == CLM_DT_BF16)
        out[i] = to_float(reinterpret_cast<const bf16_t*>(in)[i]);
    else if (dtype == CLM_DT_F16)
        out[i] = to_float(reinterpret_cast<const f16_t*>(in)[i]);
}

// W [n][k] fp32 -> MFMA fragment order of `prec` (the GEMM kernels, the 16-bit tail) / the fused exact tail's order, plain or hi + lo
int pack_gemm(clm_handle* h, int prec, const float* w, int n, int k, DevBuf& out, hipStream_t st) {
    HIPCHK(h, out.alloc(packed_weight_bytes(prec, n, k)));
    HIPCHK(h, hipMemsetAsync(out.get(), 0, out.bytes(), st));
    launch_pack_weight(prec, w, out.get(), n, k, st);
    return CLM_OK;
}
int pack_tail(clm_handle* h, bool x3, const float* w, int n, int k, DevBuf& out, hipStream_t st) {
    HIPCHK(h, out.alloc((size_t)n * k * 4));
    (x3 ? launch_pack_x3 : launch_pack_f32t)(w, out.get(), n, k, st);
    return CLM_OK;
}

// The arithmetic a chunk of L-token reads runs in.  fp16c keeps fp16 activation operands; their roundings are independent
// from token to token and average out in the attention pooling like 1/sqrt(L) (measured max |dlogit| at 3x head scale:
// 1.6e-4 at 8193 tokens, 5.6e-4 at 1000, 1.5e-3 at 100), so reads too short to average them take the exact-fp32 kernels --
// they are cheap there -- and the mode stays within the reference's 1e-3 at every length.
int mode_prec(const clm_handle* h, int L) { return (h->cfg.precision == PREC_F16C && L < h->f16c_min_len) ? (int)PREC_F32 : h->cfg.precision; }
int effective_prec(const clm_handle* h, int L) {
    if (h->run.force_prec >= 0) return h->run.force_prec;
    return h->run.fallback > 0 ? (int)PREC_F32 : mode_prec(h, L);
}
// Does the fp32 path of this handle multiply hi + lo halfs (three fp16 MFMAs per product, tail32.hip AR_X3) right now?  An fp16x3
// handle: unless told to fall back; a 16-bit handle (short reads of fp16c, fall-back level 1): unless told to fall back all the
// way (level 2).  Never inside the referee pass of a self-check, never on an fp32 handle.
bool fp32_path_is_x3(const clm_handle* h) {
    if (h->run.referee || !(h->x3_wmax < X3_WEIGHT_LIMIT)) return false;   // (weights beyond the packing's range: exact fp32 instead)
    if (h->x3) return h->run.fallback == 0;
    return h->cfg.precision != PREC_F32 && h->run.fallback < 2;
}
bool is_exact(const clm_handle* h) { return h->cfg.precision == PREC_F32 && !h->x3; }   // the handle IS its own referee
bool stop_here(const clm_handle* h, int layer, int stage) { return h->stop_layer == layer && h->stop_stage == stage; }

// Everything the engine decides about a chunk of Bc reads of L tokens, each decision once and under one name (plan_chunk says what
// each means).  The stages read these fields; none looks at the precision, the CLM_DEBUG switches or the kind of a debug stop again.
struct ChunkPlan {
    int Bc, L, prec, Lp, Lmain, S, nt128, nt_pool;
    size_t es;
    bool tuned16, fused16, fused32, fused, unfused32, alt32, x3, mlpc, lo, keep_lo;
    bool id_conv, id_resid, peel, zgated, hreg, pad_skip, seg_tables, seg_skip[NLAYER];
};

ChunkPlan plan_chunk(const clm_handle* h, int Bc, int L) {
    ChunkPlan p{};
    const bool stop = h->stop_stage >= 0;                     // a debug stop wants an intermediate: no fused tail
    p.Bc = Bc; p.L = L;
    p.prec = effective_prec(h, L);                            // (honours the self-check's referee pass and the fallback)
    p.es = elem_size(p.prec);                                 // bytes per element of z / y
    p.Lp = round_up(L, LP_ALIGN);
    p.S = conv_segments_for(L);                               // segments of the long convolution (1: one shot)
    p.alt32 = p.prec != h->cfg.precision;                     // fp16c engine, short reads: exact-fp32 kernels and packing
    p.tuned16 = p.prec != PREC_F32;
    // 16-bit modes, no debug stop: every block's tail kernel goes on, on the tile it has just produced, with LayerNorm-1 + in_proj
    // of the next block (the last block: ln_f + attention scores + pooling partials): no separate in_proj / score launches
    p.fused16 = p.tuned16 && !stop;
    // exact fp32: one fused kernel per block tail, the next block's in_proj included (tail32.hip), unless a debug stop wants an
    // intermediate or CLM_DEBUG=unfused_fp32 asks; then the separate GEMM kernels of rounds 1-3, with fc1's output in HBM
    p.fused32 = !p.tuned16 && !h->unfused_fp32 && !stop;
    p.unfused32 = !p.tuned16 && !p.fused32;
    p.fused = p.fused16 || p.fused32;
    p.x3 = p.fused32 && fp32_path_is_x3(h);                   // fp16x3: hi + lo halfs in the fused tails (the referee pass: exact)
    // reads of 128 k + 1 tokens (every 8k-bp read: 8192 bases + [SEP]): the last token would be a tile of its own, a whole extra
    // round of the tail kernel for one token per read; it is causally isolated, so a per-read matrix-vector kernel takes it
    p.peel = p.fused16 && !h->no_lone_peel && L > 128 && L % 128 == 1;
    p.Lmain = p.peel ? L - 1 : L;                             // tokens the 128-token tiles cover
    // ... and hands z over in the form the convolution reads: x0f and g = x1f * vf, filtered and gated by the in_proj stage itself
    // (two rows per channel instead of three; gemm16.hip inproj_blocks_gated)
    p.zgated = p.fused16 && !h->raw_z;
    // fp16c, round 4: y (every block) and the gated rows of z carry one lo byte per element next to the halfs; the workspace of an
    // fp16c handle keeps y's lo plane whatever a chunk runs in; second level: fc1 / fc2 as hi + lo too
    p.lo = p.prec == PREC_F16C;
    p.keep_lo = h->cfg.precision == PREC_F16C;
    p.mlpc = p.lo && h->mlp_lo;
    // 16-bit modes: block 0's in_proj output is a function of the token id alone, the convolution looks it up (ztab), single-shot
    // and segmented kernel alike, and no in_proj is launched -- unless a debug stop asks for z itself or CLM_DEBUG=no_idconv
    // (id_conv).  Without a debug stop block 0 never touches the fp32 embedding rows in HBM either: its residual is gathered from
    // the embedding table by its tail kernel (id_resid); the separate kernels a debug stop brings read the residual stream in HBM,
    // which is the one case where the two differ.  Exact fp32 with the fused tail, single-shot convolution: the same table -- it
    // is fp32 -- and h is first written by block 0's tail kernel, as in the 16-bit id path
    p.id_conv = !h->no_idconv && ((p.tuned16 && !stop_here(h, 0, CLM_STAGE_INPROJ)) || (p.fused32 && p.S == 1));
    p.id_resid = !h->no_idconv && (p.fused16 || (p.fused32 && p.S == 1));
    // The fused 16-bit tail kernels hand h from launch to launch inside each 128-token tile's own 128 KiB in the order of the
    // accumulator registers (gemm16.hip HREG): the lane that stores a value is the lane that loads it one launch later.  Whole tiles
    // only (a partial last tile's block would run into the next read's rows), and only where block 0 gathers its residual from the
    // embedding table, so that no launch of the forward reads rows another kernel wrote; every launch of a forward agrees
    p.hreg = p.fused16 && p.id_resid && !h->row_h && p.Lmain % 128 == 0;
    // Round 5: tiles wholly inside a read's [PAD] prefix are not computed, their rows come from the all-[PAD] table (pad_prefix.hip).
    // In the fused paths only (the debug / unfused paths keep computing everything), never inside the forward that fills a table,
    // and only for reads long enough to hold a whole prefix tile next to a real token.
    p.pad_skip = !h->no_pad_skip && !h->run.capture && L >= 256 && p.fused;
    p.seg_tables = p.tuned16 && !h->no_seg_skip;              // (the 16-bit fused path's segmented convolution skips prefix segments)
    // does block j's (segmented) convolution leave out the segments inside the [PAD] prefix of both reads of a pair (SegPrefix)?
    // Block 0 looks z up by token id, the others read the gated hand-over (and the table must hold them: ChunkCtx::seg_skip)
    for (int j = 0; j < NLAYER; ++j) p.seg_skip[j] = p.pad_skip && p.S > 1 && p.fused16 && (j == 0 ? p.id_resid : p.zgated);
    // tiles of a read: 128 tokens in the 16-bit tail kernel; pooling partials: one per such tile, or per T32_TILE = 64 tokens (exact tail)
    p.nt128 = tiles_of(L, 128);
    p.nt_pool = p.tuned16 ? p.nt128 : tiles_of(L, T32_TILE);
    return p;
}

// The weights of a chunk under its plan.  The GEMM kernels and the 16-bit tail: the mode's packing, or the exact-fp32 one a 16-bit
// handle keeps next to it; the fused exact tail: plain fp32 or hi + lo halfs; the 16-bit tail's two MLP products: hi + lo when asked
const Packing& gemm_packing(const clm_handle* h, const ChunkPlan& p) { return p.alt32 ? h->pk_f32 : h->pk_mode; }
const Packing& tail_packing(const clm_handle* h, const ChunkPlan& p) { return p.x3 ? h->pk_x3 : h->pk_t32; }
BlockW block_weights(const clm_handle* h, const ChunkPlan& p, int i) {
    const Packing &g = gemm_packing(h, p), &m = p.mlpc ? h->pk_mlpc : g, &t = tail_packing(h, p);
    return {&h->blk[i], g.w[i][0].get(), g.w[i][1].get(), m.w[i][2].get(), m.w[i][3].get(),
            t.w[i][0].get(), t.w[i][1].get(), t.w[i][2].get(), t.w[i][3].get()};
}

// The per-chunk workspace: buffers grown each on its own -- a call needs Bc x (its own length) of each, and chunk_for() bounds that
// product whatever the read length, so a handle that has seen 256 x 8k-token and 32 x 32k-token batches holds the larger of the two
// needs per buffer, not 256 x 32k (the round-2 shape bookkeeping did).
int ensure_workspace(clm_handle* h, const ChunkPlan& p, hipStream_t st) {
    const size_t es = p.es, Lp = (size_t)p.Lp, nb = (size_t)p.Bc, nl = (size_t)p.L, S = p.S > 1 ? (size_t)p.S : 0;
    struct { DevBuf& buf; size_t need; bool zero; } ws[] = {   // zero: padding columns [L, Lp) must never hold NaN garbage
        {h->h, nb * nl * D * 4, false},
        {h->z, nb * D3 * Lp * es, true},
        {h->y, nb * D * Lp * es, true},
        {h->u, p.unfused32 ? nb * DI * nl * es : 0, false},   // the 1024-wide fc1 output: unfused fp32 path only
        {h->scores, nb * nl * 4, false},
        {h->stats, nb * 2 * 4, false},
        // pooling partials: [POOL_SPLIT][4][256] per read (unfused fp32 path) or one POOL_PSTRIDE row per tile -- 128 tokens in the
        // 16-bit tail kernel, T32_TILE = 64 in the exact / fp16x3 one
        {h->partial, nb * std::max((size_t)POOL_SPLIT * 4 * D, (size_t)tiles_of(p.L, T32_TILE) * POOL_PSTRIDE) * 4, false},
        {h->pooled, nb * D * 4, false},
        {h->gscratch, ((nb + 1) / 2) * D * S * 16384 * sizeof(float2), false},
        {h->ids8, nb * Lp, false},
        {h->lone_ws, lone_token_ws_floats((int)nb) * 4, false},
        {h->edge_read, nb * D3 * sizeof(float2), false},
        {h->ylo, p.keep_lo ? nb * D * Lp : 0, true},
        {h->pad_p0, 3 * nb * sizeof(int), false},                     // p0 | pair order | pair partner (pad_prefix.hip)
        {h->tile_list, (1 + nb * (size_t)p.nt128) * sizeof(int), false},
    };
    bool grow = false;
    for (auto& w : ws) grow |= w.need > w.buf.bytes();
    if (!h->edge_bnd) HIPCHK(h, h->edge_bnd.alloc((size_t)1024 * 2 * D3 * sizeof(float2)));   // >= any grid (one workgroup per CU)
    if (!grow) return CLM_OK;
    HIPCHK(h, hipStreamSynchronize(st));
    for (auto& w : ws) {
        if (w.need <= w.buf.bytes()) continue;
        HIPCHK(h, w.buf.reserve(w.need));
        if (w.zero) HIPCHK(h, hipMemset(w.buf.get(), 0, w.need));
    }
    return CLM_OK;
}

int ensure_filters(clm_handle* h, int L, hipStream_t st, FilterSet** out, const ReversedFilter** krev_out) {
    *krev_out = nullptr;
    const int S = conv_segments_for(L);
    const int logn = S > 1 ? 14 : conv_logn_for(L);
    if (logn < 0 || L > h->cfg.max_seq_len)
        return fail(h, CLM_E_UNSUPPORTED, "sequence length " + std::to_string(L) + " tokens exceeds max_seq_len " +
                                              std::to_string(h->cfg.max_seq_len));
    const int key = S > 1 ? KEY_LONG : logn;
    FilterSet* fs = nullptr;
    for (auto& f : h->filters)
        if (f.key == key) fs = &f;
    const int N = 1 << logn;
    if (!fs) {
        HIPCHK(h, hipStreamSynchronize(st));
        FilterSet f;
        f.key = key;
        f.logn = logn;
        f.Lf = S > 1 ? h->cfg.max_seq_len : std::min(N / 2 + 1, h->cfg.max_seq_len);
        f.KS = S > 1 ? conv_segments_for(h->cfg.max_seq_len) : 1;
        DevBuf scratch;
        HIPCHK(h, scratch.alloc((size_t)D * N * sizeof(double2)));
        HIPCHK(h, f.tw.alloc((size_t)(N / 2) * sizeof(float2)));
        launch_twiddles(f.tw.get<float2>(), logn, st);
        for (int i = 0; i < NLAYER; ++i) {
            HIPCHK(h, f.ktime[i].alloc((size_t)f.Lf * D * 4));
            HIPCHK(h, f.kf[i].alloc((size_t)D * f.KS * N * sizeof(float2)));
            float* const kt = f.ktime[i].get<float>();
            float2* const kf = f.kf[i].get<float2>();
            const BlockF32& b = h->blk[i];
            launch_filter(b.pos_z, b.pos_t, b.f_w0, b.f_b0, b.f_freq, b.f_w2, b.f_b2, b.f_w4, b.f_b4, b.f_w6, b.deltas, kt, f.Lf, st);
            if (S == 1) {
                launch_filter_spectrum(kt, b.filt_bias, kf, scratch.get<double2>(), f.Lf, logn, 0, f.Lf, -1, st);
                if (logn == 14) {                            // (round 5: the exact / fp16x3 engine's fp32 rows take the persistent kernel too)
                    HIPCHK(h, f.kfp[i].alloc((size_t)D * N * sizeof(float2)));
                    launch_spectrum_lanepack(kf, f.kfp[i].get<float2>(), 1, 0, st);
                }
            } else {   // kf [256][KS][N], lane-packed for the segmented kernel: one launch per partition, through a temporary
                DevBuf tmp;
                HIPCHK(h, tmp.alloc((size_t)D * N * sizeof(float2)));
                for (int j = 0; j < f.KS; ++j) {
                    launch_filter_spectrum(kt, b.filt_bias, tmp.get<float2>(), scratch.get<double2>(), f.Lf, logn, j * SEG_LEN,
                                           SEG_LEN, (j - 1) * SEG_LEN, st);
                    launch_spectrum_lanepack(tmp.get<float2>(), kf, f.KS, j, st);
                }
                HIPCHK(h, hipStreamSynchronize(st));         // (before `tmp` is freed)
            }
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(st));                 // (before `scratch` is freed)
        h->filters.push_back(std::move(f));
        fs = &h->filters.back();
    }
    if (conv_lone_tail(L)) {               // the reversed taps [0, L) of the dot product for the lone last token
        for (auto& r : fs->krev)
            if (r.L == L) *krev_out = &r;
        if (!*krev_out) {
            ReversedFilter r;
            r.L = L;
            r.stride = round_up(L, 8);
            for (int i = 0; i < NLAYER; ++i) {
                HIPCHK(h, r.p[i].alloc((size_t)D * r.stride * 4));
                launch_filter_reversed(fs->ktime[i].get<float>(), h->blk[i].filt_bias, r.p[i].get<float>(), L, r.stride, st);
            }
            fs->krev.push_back(std::move(r));
            *krev_out = &fs->krev.back();
        }
    }
    *out = fs;
    return CLM_OK;
}

// Asynchronous error of an EARLIER forward (the call itself returned before its kernels ran): reported once, by the next
// forward / stage_wait / profile_read / clm_check call.  The reference raises IndexError inside nn.Embedding for such ids.
int check_bad_ids(clm_handle* h) {
    if (h->bad_ids && *reinterpret_cast<volatile int*>(h->bad_ids)) {
        *reinterpret_cast<volatile int*>(h->bad_ids) = 0;
        return fail(h, CLM_E_INVALID, "an earlier batch held token ids outside [0, " + std::to_string(h->cfg.vocab_rows) +
                                          ") (its logits were computed with those ids clamped; the reference raises IndexError)");
    }
    return CLM_OK;
}

// Reads pushed through all layers together: cfg.chunk_reads, capped by tokens so that a chunk's workspace stays bounded whatever
// the read length -- 256 x 8,256 tokens in the 16-bit modes (z + y + h: 6.5 GB; measured round 3, same box: 7,976 / 8,047 / 8,164
// reads/s at 64 / 128 / 256 reads per chunk: the ~26 small launches of a chunk, the persistent kernels' ramps and the head are paid
// per chunk, and 288 GB of HBM have room), a quarter of that in exact fp32 (its 1024-wide fc1 output is 4 KiB per token, and the
// proven size).  Even, so that a chunk boundary never splits a read pair of the packed transform.
int chunk_for(const clm_handle* h, int L) {
    // (exact fp32 with the fused tail has no fc1 output in HBM either: the same cap as the 16-bit modes)
    const long long cap_tokens = plan_chunk(h, 1, L).unfused32 ? 64LL * 8256 : 256LL * 8256;
    long long c = cap_tokens / round_up(L, LP_ALIGN);
    if (c > h->cfg.chunk_reads) c = h->cfg.chunk_reads;
    if (c > TILE_LIST_MAX_READS) c = TILE_LIST_MAX_READS;     // (a tile-list entry holds its read in 12 bits)
    if (c > 1) c &= ~1LL;
    return c < 1 ? 1 : (int)c;
}

int forward_chunk(clm_handle* h, const void* ids, int ids_dtype, int64_t row_stride, int Bc, int L, float* logits, hipStream_t st,
                  const clm_attn_out* attn = nullptr, int b0 = 0, const clm_traj_out* traj = nullptr);

// The all-[PAD] table of the arithmetic the reads of this chunk run in (pad_prefix.hip), long enough for its L tokens: built on
// first use -- ONE forward of one all-[PAD] read through this very engine, with the stages' capture hooks copying out what the
// later stages read of it -- and kept until the weights change.  Lengths come in classes (1,025 ... 32,769 tokens, then
// max_seq_len) so that a file of ragged batches builds at most a handful.  The values at position t do not depend on the length of
// the read they were computed in (causal backbone, taps independent of L) beyond the rounding of its transform size.
int ensure_pad_table(clm_handle* h, const ChunkPlan& p, hipStream_t st, clm_handle::PadTable** out) {
    const auto same = [&p](const clm_handle::PadTable& t) { return t.prec == p.prec && t.x3 == p.x3 && t.mlp_lo == p.mlpc; };
    size_t old = 0;                                          // the table of this arithmetic, if there is one
    while (old < h->pad_tables.size() && !same(h->pad_tables[old])) ++old;
    if (old < h->pad_tables.size() && h->pad_tables[old].L >= p.L) { *out = &h->pad_tables[old]; return CLM_OK; }
    int LT = 1025;
    while (LT < p.L && LT < 32769) LT = 2 * (LT - 1) + 1;
    if (LT < p.L) LT = h->cfg.max_seq_len;
    if (LT > h->cfg.max_seq_len) LT = h->cfg.max_seq_len;
    if (LT < p.L) return fail(h, CLM_E_INVALID, "ensure_pad_table: read longer than max_seq_len");
    HIPCHK(h, hipStreamSynchronize(st));
    if (old < h->pad_tables.size()) h->pad_tables.erase(h->pad_tables.begin() + (long)old);   // a shorter one is replaced
    clm_handle::PadTable t;
    t.prec = p.prec; t.x3 = p.x3; t.mlp_lo = p.mlpc;
    t.L = LT; t.Lp = round_up(LT, LP_ALIGN);
    for (int i = 1; i < NLAYER; ++i) HIPCHK(h, t.z[i].alloc((size_t)D3 * t.Lp * p.es));
    // (the exact path: partials per 64-token tile, and the final residual rows as well -- clm_debug_fetch("hidden") shows them)
    if (!p.tuned16) HIPCHK(h, t.hfin.alloc((size_t)LT * D * 4));
    HIPCHK(h, t.scores.alloc((size_t)LT * 4));
    HIPCHK(h, t.partial.alloc((size_t)tiles_of(LT, T32_TILE) * POOL_PSTRIDE * 4));
    t.S = conv_segments_for(LT);
    if (t.S > 1 && p.seg_tables)
        for (int i = 0; i < NLAYER; ++i) {
            HIPCHK(h, t.gspec[i].alloc((size_t)D * t.S * 16384 * sizeof(float2)));
            HIPCHK(h, t.dots[i].alloc((size_t)D * (t.S - 1) * SEG_DOT_THREADS * 4));
            HIPCHK(h, hipMemsetAsync(t.dots[i].get(), 0, t.dots[i].bytes(), st));
        }
    if ((size_t)t.Lp > h->pad_ids.bytes()) {
        HIPCHK(h, h->pad_ids.reserve((size_t)t.Lp));
        HIPCHK(h, hipMemsetAsync(h->pad_ids.get(), PAD_ID, (size_t)t.Lp, st));
    }
    if (!h->pad_logits) HIPCHK(h, h->pad_logits.alloc(NCLS * 4));
    h->pad_tables.push_back(std::move(t));
    clm_handle::PadTable* tp = &h->pad_tables.back();
    int rc;
    {
        RunScope<clm_handle> scope(h);
        h->run.force_prec = p.prec;                          // (fp16c: the class length may lie on the other side of the length switch)
        h->run.capture = tp;
        rc = forward_chunk(h, h->pad_ids.get(), CLM_DT_U8, tp->Lp, 1, LT, h->pad_logits.get<float>(), st);
    }
    if (rc) {
        h->pad_tables.pop_back();
        return rc;
    }
    *out = tp;
    return CLM_OK;
}

// ---- the stages of a chunk's forward, free functions over ChunkCtx.  STOPPED: the debug stop (clm_debug_stop_after) sits right
// behind the stage that returns it, and forward_chunk ends there with CLM_OK (the error codes are negative)
constexpr int STOPPED = 1;

struct ChunkCtx {
    clm_handle* const h;
    const ChunkPlan p;
    const hipStream_t st;
    FilterSet* fs = nullptr;
    const ReversedFilter* kr = nullptr;            // lone-tail lengths only
    clm_handle::PadTable* ptab = nullptr;          // p.pad_skip only; (workspace pointers are taken where used: they may move until the table is there)
    unsigned char* ylo() const { return p.lo ? h->ylo.get<unsigned char>() : nullptr; }
    // (with segment skipping the pairs of the segmented convolutions are formed by descending prefix: perm / partner live behind p0)
    int* pair_perm() const { return h->pad_p0.get<int>() + p.Bc; }
    int* pair_partner() const { return h->pad_p0.get<int>() + 2 * p.Bc; }
    // reads of S * 8192 + 1 tokens carry the last token's dot product through the segments: its table sums belong to ONE length
    bool seg_skip(int j) const { return p.seg_skip[j] && ptab->gspec[j] && (!kr || p.L == ptab->L); }
};

// points of a trajectory with stride S along rows of L tokens
int traj_points(int L, int S) { return (L + S - 1) / S; }

// the workspace sized for this chunk (and for its trajectory request, if there is one)
int size_workspace(ChunkCtx& c, const clm_traj_out* traj = nullptr) {
    auto& [h, p, st, fs, kr, ptab] = c;
    if (int rc = ensure_workspace(h, p, st)) return rc;
    if (traj) {
        if (int rc = grow(h, Sync::Stream(st), {{&h->traj_pooled, (size_t)p.Bc * traj_points(p.L, traj->stride) * D * 4},
                                                {&h->traj_npad, (size_t)p.Bc * 4}}))
            return rc;
    }
    h->last_B = p.Bc; h->last_L = p.L; h->last_Lp = p.Lp;
    h->last_hreg_Lmain = p.hreg ? p.Lmain : 0;
    h->rows.valid = false;                   // (this chunk rewrites the residual rows: whoever held them must not read them again)
    ++h->rows.generation;
    if (h->ws_es != p.es) {                  // fp16c: fp32 and fp16 chunks share z / y -- what one type left in the padding
        if (h->ws_es) {                      // columns may read as NaN in the other
            HIPCHK(h, hipMemsetAsync(h->z.get(), 0, h->z.bytes(), st));
            HIPCHK(h, hipMemsetAsync(h->y.get(), 0, h->y.bytes(), st));
        }
        h->ws_es = p.es;
    }
    return CLM_OK;
}

// short filter + gate + long convolution, one shot or segmented; idconv: z comes from the id table
int stage_conv(ChunkCtx& c, int i, const BlockW& w, bool idconv) {
    auto& [h, p, st, fs, kr, ptab] = c;
    clm_handle::PadTable* const cap = h->run.capture;
    StageTimer t(h, st, CLM_STAGE_CONV);
    const unsigned char* ids8 = idconv ? h->ids8.get<unsigned char>() : nullptr;
    const float* ztab = idconv ? h->ztab.get<float>() : nullptr;
    const int flags = h->conv_flags | ((p.zgated && i > 0) ? CONV_GATED : 0);
    if (p.S == 1) {
        launch_hyena_conv(p.prec, h->z.get(), h->y.get(), fs->kf[i].get<float2>(), fs->tw.get<float2>(), fs->ktime[i].get<float>(), w.f->short_w, w.f->short_b,
                          p.Bc, p.L, p.Lp, fs->logn, ids8, ztab, st, flags, fs->kfp[i].get<float2>(), c.ylo());
        return CLM_OK;
    }
    // [PAD]-prefix reuse: segments inside the prefix of both reads of a pair come from the table (SegPrefix)
    SegPrefix pfx;
    if (cap && cap->gspec[i]) {
        pfx.dots_out = kr ? cap->dots[i].get<float>() : nullptr;
        pfx.dots_segs = cap->S - 1;
    } else if (c.seg_skip(i)) {
        pfx.p0 = h->pad_p0.get<int>();
        pfx.perm = c.pair_perm();
        pfx.tab = ptab->gspec[i].get<float2>();
        pfx.tab_segs = ptab->S;
        pfx.dots_in = ptab->dots[i].get<float>();
        pfx.dots_segs = ptab->S - 1;
    }
    launch_hyena_conv_seg(p.prec, h->z.get(), h->y.get(), fs->kf[i].get<float2>(), fs->KS, fs->tw.get<float2>(), w.f->short_w, w.f->short_b, h->gscratch.get<float2>(),
                          p.Bc, p.L, p.Lp, p.S, kr ? kr->p[i].get<float>() : nullptr, kr ? kr->stride : 0, ids8, ztab, st, flags, c.ylo(), pfx);
    if (cap && cap->gspec[i]) {   // (one read = pair 0: [256][S][N] at the head of the scratch), then pair form
        HIPCHK(h, hipMemcpyAsync(cap->gspec[i].get<float2>(), h->gscratch.get<float2>(), (size_t)D * p.S * 16384 * sizeof(float2), hipMemcpyDeviceToDevice, st));
        launch_spectra_pair_form(cap->gspec[i].get<float2>(), p.S, st);
    }
    return CLM_OK;
}

// The [PAD] prefix behind a fused tail: what block i leaves for the next stage -- z of nrow16 element rows + nlo byte rows, or the last
// block's pooling scores and partials (exact path: its residual rows too) -- copied out of (capture) or in from (pad_skip) the table
int prefix_hooks(ChunkCtx& c, int i, int nrow16, int nlo) {
    auto& [h, p, st, fs, kr, ptab] = c;
    clm_handle::PadTable* const cap = h->run.capture;
    int* const p0 = h->pad_p0.get<int>();
    float *const scores = h->scores.get<float>(), *const partial = h->partial.get<float>();
    const bool last = i + 1 == NLAYER;
    if (cap) {
        if (!last) HIPCHK(h, hipMemcpyAsync(cap->z[i + 1].get(), h->z.get(), (size_t)D3 * p.Lp * p.es, hipMemcpyDeviceToDevice, st));
        else {
            if (!p.tuned16) HIPCHK(h, hipMemcpyAsync(cap->hfin.get<float>(), h->h.get<float>(), (size_t)p.L * D * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(cap->scores.get<float>(), scores, (size_t)p.L * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(cap->partial.get<float>(), partial, (size_t)p.nt_pool * POOL_PSTRIDE * 4, hipMemcpyDeviceToDevice, st));
        }
    } else if (p.pad_skip) {
        if (!last)                    // (rows of segments the next convolution will not read are not copied)
            launch_prefix_fill_z(p0, h->z.get(), ptab->z[i + 1].get(), p.Bc, p.Lp, ptab->Lp, p.Lmain, (int)p.es, nrow16, nlo, st,
                                 c.seg_skip(i + 1) ? p.S : 0, p.tuned16 ? c.pair_partner() : nullptr);
        else {
            if (!p.tuned16) launch_prefix_fill_h(p0, h->h.get<float>(), ptab->hfin.get<float>(), p.Bc, p.L, p.L, st);
            launch_prefix_fill_pool(p0, scores, partial, ptab->scores.get<float>(), ptab->partial.get<float>(), p.Bc, p.L, p.nt_pool, p.Lmain, st,
                                    p.tuned16 ? 1 : 128 / T32_TILE);   // (partials per 128 tokens)
        }
    }
    return CLM_OK;
}

// 16-bit block tail: out_proj + LN2 + fc1 + GELU + fc2 + both residuals in one kernel (tail16_kernel), with the next block's
// LN1 + in_proj or, after the last block, ln_f + scores + pooling partials when fused; then the gated patch, the lone token
// (fp32 matrix-vector products on the fp32 originals, lone_token.hip) and the [PAD] prefix
int tail16(ChunkCtx& c, int i, const BlockW& w) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const BlockF32& f = *w.f;
    const NetF32& n = h->net;
    const bool last = i + 1 == NLAYER;
    StageTimer t(h, st, CLM_STAGE_TAIL);
    const ScorePoolArgs spa{h->h.get<float>(), n.lnf_g, n.lnf_b, gemm_packing(h, p).score.get(), n.att_b1, n.att_w2, n.att_b2,
                            h->scores.get<float>(), h->partial.get<float>(), p.Bc, p.L, p.nt128, h->cfg.ln_eps};
    TailArgs ta{h->y.get(), h->h.get<float>(), w.w_out, w.w_fc1, w.w_fc2, f.b_out, f.ln2_g, f.ln2_b, f.b_fc1, f.b_fc2, p.Bc, p.L, p.Lp,
                h->cfg.ln_eps, p.Lmain, (p.id_resid && i == 0) ? h->ids8.get<unsigned char>() : nullptr, n.emb,
                nullptr, nullptr, nullptr, nullptr, nullptr, spa};
    ta.ylo = c.ylo();
    ta.mlp_lo = p.mlpc;
    ta.hreg = p.hreg;
    ta.tiles = h->tile_list.get<int>();
    const BlockF32* nf = last ? nullptr : &h->blk[i + 1];
    if (p.fused16 && !last) {
        ta.n_w = block_weights(h, p, i + 1).w_in; ta.n_bias = nf->b_in; ta.n_g = nf->ln1_g; ta.n_b = nf->ln1_b; ta.n_z = h->z.get();
        if (p.zgated) {
            ta.zg = 1; ta.n_fir = h->fir[i + 1].get<float4>(); ta.edge_bnd = h->edge_bnd.get<float2>();
            ta.edge_read = p.peel ? h->edge_read.get<float2>() : nullptr;
            ta.zlo = p.lo;
        }
    }
    launch_tail16(p.prec, ta, !p.fused16 ? NEXT_NONE : (last ? NEXT_SCORE : NEXT_INPROJ), st);
    if (ta.zg) launch_gated_patch(p.prec, ta, st);          // tokens 0, 1 of the workgroup ranges that start inside a read
    if (p.peel) {
        LoneTokenArgs la{};
        la.y = h->y.get(); la.h = h->h.get<float>(); la.ids8 = ta.ids8; la.emb = ta.emb;
        la.w_out = f.w[1]; la.b_out = f.b_out; la.ln2_g = f.ln2_g; la.ln2_b = f.ln2_b;
        la.w_fc1 = f.w[2]; la.b_fc1 = f.b_fc1; la.w_fc2 = f.w[3]; la.b_fc2 = f.b_fc2;
        la.last = last;
        if (last) {
            la.n_g = n.lnf_g; la.n_b = n.lnf_b;
            la.att_w1 = n.att_w1; la.att_b1 = n.att_b1; la.att_w2 = n.att_w2; la.att_b2 = n.att_b2;
            la.scores = h->scores.get<float>(); la.partial = h->partial.get<float>();
        } else {
            la.n_g = nf->ln1_g; la.n_b = nf->ln1_b; la.n_w = nf->w[0]; la.n_bias = nf->b_in; la.n_z = h->z.get();
            if (ta.zg) { la.n_fir = ta.n_fir; la.edge_read = h->edge_read.get<float2>(); }
        }
        la.ws = h->lone_ws.get<float>();
        la.B = p.Bc; la.L = p.L; la.Lp = p.Lp; la.ntiles = p.nt128; la.eps = h->cfg.ln_eps;
        la.ylo = c.ylo(); la.zlo = ta.zlo;
        launch_lone_token(p.prec, la, st);
    }
    return p.fused16 ? prefix_hooks(c, i, ta.zg ? 2 * D : D3, ta.zlo ? 2 * D : 0) : CLM_OK;
}

// exact fp32 / fp16x3 block tail (tail32.hip), the next block's in_proj or -- the last block -- ln_f + pooling scores + per-tile
// pooling partials on the tile still on chip (T32_SCORE); then the [PAD] prefix
int tail32(ChunkCtx& c, int i, const BlockW& w) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const BlockF32& f = *w.f;
    const NetF32& n = h->net;
    StageTimer t(h, st, CLM_STAGE_TAIL);
    const bool last = i + 1 == NLAYER;
    const BlockF32* nf = last ? nullptr : &h->blk[i + 1];
    const Tail32Score ts{tail_packing(h, p).score.get(), n.att_b1, n.att_w2, n.att_b2, n.lnf_g, n.lnf_b, h->scores.get<float>(), h->partial.get<float>()};
    launch_tail32(h->y.get<float>(), h->h.get<float>(), w.t_out, w.t_fc1, w.t_fc2, last ? nullptr : block_weights(h, p, i + 1).t_in, f.b_out,
                  f.b_fc1, f.b_fc2, last ? nullptr : nf->b_in, f.ln2_g, f.ln2_b, last ? nullptr : nf->ln1_g, last ? nullptr : nf->ln1_b,
                  h->z.get<float>(), p.Bc, p.L, p.Lp, h->cfg.ln_eps, st, p.x3, p.pad_skip ? h->pad_p0.get<int>() : nullptr, last ? &ts : nullptr,
                  (i == 0 && p.id_resid) ? h->ids8.get<unsigned char>() : nullptr, n.emb);
    return prefix_hooks(c, i, D3, 0);
}

// the separate kernels: a debug stop after out_proj (16-bit modes), the unfused exact-fp32 path
int tail_unfused(ChunkCtx& c, int i, const BlockW& w) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const BlockF32& f = *w.f;
    {
        StageTimer t(h, st, CLM_STAGE_OUTPROJ);
        if (p.tuned16) launch_outproj16(p.prec, h->y.get(), w.w_out, f.b_out, h->h.get<float>(), p.Bc, p.L, p.Lp, st);
        else launch_outproj(h->y.get(), w.w_out, f.b_out, h->h.get<float>(), p.Bc, p.L, p.Lp, st);
    }
    if (stop_here(h, i, CLM_STAGE_OUTPROJ)) return STOPPED;
    {
        StageTimer t(h, st, CLM_STAGE_FC1);
        launch_fc1(h->h.get<float>(), f.ln2_g, f.ln2_b, w.w_fc1, f.b_fc1, h->u.get(), p.Bc, p.L, h->cfg.ln_eps, st);
    }
    if (stop_here(h, i, CLM_STAGE_FC1)) return STOPPED;
    StageTimer t(h, st, CLM_STAGE_FC2);
    launch_fc2(h->u.get(), w.w_fc2, f.b_fc2, h->h.get<float>(), p.Bc, p.L, st);
    return CLM_OK;
}

// One Hyena block: in_proj (when no tail kernel has done it and no table holds it), convolution, tail
int run_block(ChunkCtx& c, int i) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const BlockW w = block_weights(h, p, i);
    const bool idconv = i == 0 && p.id_conv;
    if (!idconv && !(p.fused && i > 0)) {
        StageTimer t(h, st, CLM_STAGE_INPROJ);
        if (p.tuned16) launch_inproj16(p.prec, h->h.get<float>(), w.f->ln1_g, w.f->ln1_b, w.w_in, w.f->b_in, h->z.get(), p.Bc, p.L, p.Lp, h->cfg.ln_eps, st);
        else launch_inproj(h->h.get<float>(), w.f->ln1_g, w.f->ln1_b, w.w_in, w.f->b_in, h->z.get(), p.Bc, p.L, p.Lp, h->cfg.ln_eps, st);
    }
    if (stop_here(h, i, CLM_STAGE_INPROJ)) return STOPPED;
    if (int rc = stage_conv(c, i, w, idconv)) return rc;
    if (stop_here(h, i, CLM_STAGE_CONV)) return STOPPED;
    const int rc = (p.tuned16 && !stop_here(h, i, CLM_STAGE_OUTPROJ)) ? tail16(c, i, w) : (p.fused32 ? tail32(c, i, w) : tail_unfused(c, i, w));
    if (rc) return rc;
    return (stop_here(h, i, CLM_STAGE_FC2) || (p.tuned16 && stop_here(h, i, CLM_STAGE_FC1))) ? STOPPED : CLM_OK;
}

// ln_f + attention pooling + classifier
int stage_head(ChunkCtx& c, float* logits) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const NetF32& n = h->net;
    const void* const w1 = gemm_packing(h, p).score.get();
    float *const hh = h->h.get<float>(), *const scores = h->scores.get<float>(), *const partial = h->partial.get<float>();
    const float eps = h->cfg.ln_eps;
    if (p.tuned16 && !p.fused16) {   // score + pooling partials in one pass over h, merged by the classifier kernel
        StageTimer t(h, st, CLM_STAGE_SCORE);
        launch_score_pool16(p.prec, hh, n.lnf_g, n.lnf_b, w1, n.att_b1, n.att_w2, n.att_b2, scores, partial, p.Bc, p.L, eps, st);
    }
    if (p.tuned16 || p.fused32) {    // (exact fused: scores and per-tile pooling partials came out of the last block's tail kernel)
        StageTimer t(h, st, CLM_STAGE_HEADMLP);
        launch_head_tiles(partial, p.nt_pool, h->hw, h->pooled.get<float>(), logits, p.Bc, st);
    } else {
        {
            StageTimer t(h, st, CLM_STAGE_SCORE);
            launch_score(hh, n.lnf_g, n.lnf_b, w1, n.att_b1, n.att_w2, n.att_b2, scores, p.Bc, p.L, eps, st);
        }
        {
            StageTimer t(h, st, CLM_STAGE_POOL);
            launch_softmax_stats(scores, h->stats.get<float>(), p.Bc, p.L, st);
            launch_pool(hh, n.lnf_g, n.lnf_b, scores, h->stats.get<float>(), partial, p.Bc, p.L, eps, st);
        }
        StageTimer t(h, st, CLM_STAGE_HEADMLP);
        launch_head_mlp(partial, h->hw, h->pooled.get<float>(), logits, p.Bc, st);
    }
    return launched(h, "stage_head");
}

// The chunk's attention outputs (clm_forward_attn), at the rows of its reads [b0, b0 + Bc) in the caller's buffers: one kernel behind
// the head, on the scores every path has completed by then (fused tails, separate kernels, the lone token, rows from the [PAD] table)
int stage_attn(ChunkCtx& c, const clm_attn_out& a, int b0) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const size_t r = (size_t)b0;
    launch_attn_weights(h->scores.get<float>(), h->ids8.get<unsigned char>(), p.Bc, p.L, p.Lp,
                        a.weights ? a.weights + r * (size_t)a.weights_row_stride : nullptr, a.weights_row_stride,
                        a.summary ? a.summary + r : nullptr, a.summary ? a.peak_pos + r * a.top_k : nullptr,
                        a.summary ? a.peak_weight + r * a.top_k : nullptr, a.top_k, st);
    return launched(h, "stage_attn");
}

// The chunk's running verdict (clm_forward_traj), at the rows of its reads [b0, b0 + Bc) in the caller's buffers: the prefix merge of
// the pooling partials every fused path has completed by then (tail kernels, the lone token, tiles from the [PAD] table), the
// classifier over the interior points, then the chunk's own logits into the last point and the summary (trajectory.hip)
int stage_traj(ChunkCtx& c, const clm_traj_out& t, int b0, const float* logits) {
    auto& [h, p, st, fs, kr, ptab] = c;
    const int tile = p.tuned16 ? 128 : T32_TILE, per = t.stride / tile, K = traj_points(p.L, t.stride), rows = p.Bc * (K - 1);
    if (!p.fused || p.nt_pool != tiles_of(p.L, tile) || tiles_of(p.nt_pool, per) != K || t.point_stride < K ||
        (size_t)p.Bc * K * D * 4 > h->traj_pooled.bytes() || (size_t)p.Bc * 4 > h->traj_npad.bytes())
        return fail(h, CLM_E_STATE, "stage_traj: the chunk's plan and workspace do not fit the request");   // (check_traj_arg saw to it)
    float* const out = t.logits + (size_t)b0 * t.point_stride * NCLS;
    launch_traj_prefix(h->partial.get<float>(), p.nt_pool, per, K, h->traj_pooled.get<float>(), h->ids8.get<unsigned char>(), p.L, p.Lp,
                       h->traj_npad.get<int>(), p.Bc, st);
    launch_traj_classifier(h->traj_pooled.get<float>(), K, rows, h->hw, out, t.point_stride, st);
    launch_traj_summary(logits, out, t.point_stride, p.Bc, K, t.stride, p.L, h->traj_npad.get<int>(), h->ids8.get<unsigned char>(), p.Lp,
                        t.summary ? t.summary + b0 : nullptr, st);
    return launched(h, "stage_traj");
}

int forward_chunk(clm_handle* h, const void* ids, int ids_dtype, int64_t row_stride, int Bc, int L, float* logits, hipStream_t st,
                  const clm_attn_out* attn, int b0, const clm_traj_out* traj) {
    ChunkCtx c{h, plan_chunk(h, Bc, L), st};
    const ChunkPlan& p = c.p;
    // filters of the length class, workspace, [PAD] table
    if (int rc = ensure_filters(h, L, st, &c.fs, &c.kr)) return rc;
    if (int rc = size_workspace(c, traj)) return rc;
    if (p.pad_skip) {                                        // (before this chunk's ids land in the workspace: the build runs through it)
        if (int rc = ensure_pad_table(h, p, st, &c.ptab)) return rc;
        if (int rc = size_workspace(c)) return rc;           // (the build may have regrown -- never shrunk -- the buffers; cheap when not)
        if (int rc = ensure_filters(h, L, st, &c.fs, &c.kr)) return rc;   // (... or added a filter class: the vector behind fs moved)
    }
    if (p.zgated && tail16_grid(tiles_of(p.Lmain, 128) * Bc) > 1024)
        return fail(h, CLM_E_UNSUPPORTED, "more than 1024 compute units: edge_bnd is sized for 1024 workgroups");
    // embedding rows (unless block 0 gathers them itself) and clamped ids, then the [PAD] prefixes: tile list, pair order
    unsigned char* const ids8 = h->ids8.get<unsigned char>();
    {
        StageTimer t(h, st, CLM_STAGE_EMBED);
        launch_embed(ids, ids_dtype, row_stride, h->net.emb, p.id_resid ? nullptr : h->h.get<float>(), ids8, Bc, L, p.Lp, st, h->bad_ids);
    }
    if (stop_here(h, -1, CLM_STAGE_EMBED)) return CLM_OK;
    if (p.tuned16 || p.pad_skip) launch_pad_tiles(ids8, Bc, p.Lp, p.Lmain, p.pad_skip ? 1 : 0, h->pad_p0.get<int>(), h->tile_list.get<int>(), st);
    if (p.pad_skip && p.S > 1) launch_pair_order(h->pad_p0.get<int>(), Bc, c.pair_perm(), c.pair_partner(), st);
    int rc = CLM_OK;
    for (int i = 0; i < NLAYER && !rc; ++i) rc = run_block(c, i);
    if (!rc) rc = stage_head(c, logits);
    if (!rc && attn) rc = stage_attn(c, *attn, b0);
    if (!rc && traj) rc = stage_traj(c, *traj, b0, logits);
    return rc == STOPPED ? CLM_OK : rc;
}

// The attention request of clm_forward_attn / clm_forward_staged_attn for reads of L tokens (null: none, nothing to check)
int check_attn_arg(clm_handle* h, const char* who, const clm_attn_out* a, int L) {
    if (!a) return CLM_OK;
    const std::string w(who);
    if (a->struct_size != (int32_t)sizeof(clm_attn_out)) return fail(h, CLM_E_INVALID, w + ": clm_attn_out size mismatch");
    const int n_peak_args = (a->summary != nullptr) + (a->peak_pos != nullptr) + (a->peak_weight != nullptr);
    if (n_peak_args != 0 && n_peak_args != 3)
        return fail(h, CLM_E_INVALID, w + ": summary, peak_pos and peak_weight go together (all three or none)");
    if (!a->weights && !a->summary) return fail(h, CLM_E_INVALID, w + ": the attention request asks for nothing (weights and summary are NULL)");
    if (a->summary && (a->top_k < 1 || a->top_k > ATTN_MAX_TOP_K))
        return fail(h, CLM_E_INVALID, w + ": top_k must be 1 ... " + std::to_string(ATTN_MAX_TOP_K));
    if (a->weights && a->weights_row_stride < L) return fail(h, CLM_E_INVALID, w + ": weights_row_stride is shorter than a read");
    if (L > ATTN_MAX_L)
        return fail(h, CLM_E_UNSUPPORTED, w + ": attention outputs exist for reads of up to " + std::to_string(ATTN_MAX_L) + " tokens");
    if (h->stop_stage >= 0) return fail(h, CLM_E_STATE, w + ": a debug stop is set (clm_debug_stop_after): the forward ends before the head");
    return CLM_OK;
}

// The trajectory request of clm_forward_traj / clm_forward_staged_traj for reads of L tokens (null: none, nothing to check)
int check_traj_arg(clm_handle* h, const char* who, const clm_traj_out* t, int L) {
    if (!t) return CLM_OK;
    if (int rc = check_traj_request(h, who, t, L)) return rc;   // what holds for every net; then what the Hyena engine adds
    const std::string w(who);
    if (L > ATTN_MAX_L)
        return fail(h, CLM_E_UNSUPPORTED, w + ": trajectories exist for reads of up to " + std::to_string(ATTN_MAX_L) + " tokens");
    if (h->stop_stage >= 0)
        return fail(h, CLM_E_UNSUPPORTED, w + ": a debug stop is set (clm_debug_stop_after): the forward ends before the head");
    if (!plan_chunk(h, 1, L).fused)
        return fail(h, CLM_E_UNSUPPORTED, w + ": the unfused exact path (CLM_DEBUG=unfused_fp32) leaves no per-tile pooling partials");
    return CLM_OK;
}

size_t ids_elem_size(int dtype) { return dtype == CLM_DT_I64 ? 8 : (dtype == CLM_DT_I32 ? 4 : 1); }

// `attn`, `traj`: the caller's attention and trajectory outputs for all B reads, or null -- the self-check, the [PAD]-table build and
// every other forward the engine runs for itself pass none
int forward_all(clm_handle* h, const void* ids, int ids_dtype, int64_t row_stride, int B, int L, float* logits, hipStream_t st,
                const clm_attn_out* attn = nullptr, const clm_traj_out* traj = nullptr) {
    const int chunk = chunk_for(h, L);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int Bc = B - b0 < chunk ? B - b0 : chunk;
        const char* p = reinterpret_cast<const char*>(ids) + (size_t)b0 * row_stride * ids_elem_size(ids_dtype);
        if (int rc = forward_chunk(h, p, ids_dtype, row_stride, Bc, L, logits + (size_t)b0 * NCLS, st, attn, b0, traj)) return rc;
    }
    h->rows.valid = h->stop_stage < 0;                        // (a debug stop ends the forward before the last block)
    h->rows.one_chunk = B <= chunk;
    h->rows.exact = !plan_chunk(h, B < chunk ? B : chunk, L).tuned16;
    h->rows.B = B; h->rows.L = L;
    return CLM_OK;
}

}  // namespace

// ======================================================================================== C ABI
extern "C" {

int clm_abi_version(void) { return CLM_ABI_VERSION; }

int clm_default_config(clm_config* c) {
    if (!c) return CLM_E_INVALID;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(clm_config);
    c->d_model = D; c->n_layer = NLAYER; c->d_inner = DI; c->vocab_rows = VOCAB; c->filter_order = FORDER;
    c->emb_dim = EMB; c->max_seq_len = 32770; c->head_hidden = HH; c->n_classes = NCLS;
    c->ln_eps = 1e-5f;
    c->precision = CLM_PREC_F32;
    c->chunk_reads = 256;
    return CLM_OK;
}

int clm_create(const clm_config* cfg, int device, clm_handle** out) {
    if (!cfg || !out) return fail<clm_handle>(nullptr, CLM_E_INVALID, "clm_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(clm_config)) return fail<clm_handle>(nullptr, CLM_E_INVALID, "clm_config size mismatch");
    if (cfg->d_model != D || cfg->n_layer != NLAYER || cfg->d_inner != DI || cfg->vocab_rows != VOCAB ||
        cfg->filter_order != FORDER || cfg->emb_dim != EMB || cfg->head_hidden != HH || cfg->n_classes != NCLS)
        return fail<clm_handle>(nullptr, CLM_E_UNSUPPORTED,
                                "only the HyenaDNA-small-32k + 512-wide attention-pooling head of chimeralm/models/lm.py is built");
    if (cfg->precision < CLM_PREC_F32 || cfg->precision > CLM_PREC_F16X3 || cfg->chunk_reads < 1 ||
        cfg->max_seq_len < 2)
        return fail<clm_handle>(nullptr, CLM_E_INVALID, "clm_create: bad precision / chunk_reads / max_seq_len");
    if (int rc = use_gfx950<clm_handle>(device, "clm_create")) return rc;
    clm_handle* h = new clm_handle();
    // developer switches (A/B runs, tests): ONE variable, CLM_DEBUG, a comma-separated list read when a handle is created
    // (clm_common.h debug_flag) -- no product behaviour hangs on the environment
    h->unfused_fp32 = debug_flag("unfused_fp32");      // exact fp32 through the separate GEMM kernels instead of tail32_kernel
    h->no_idconv = debug_flag("no_idconv");            // block 0's in_proj instead of the id-table convolution
    h->no_lone_peel = debug_flag("no_lone_peel");      // the lone last token of 128 k + 1-token reads in a tile of its own
    if (debug_flag("conv_oneshot")) h->conv_flags |= CONV_ONESHOT;
    if (debug_flag("conv_no_xcd")) h->conv_flags |= CONV_NO_XCD;
    h->raw_z = debug_flag("raw_z");                    // the fused in_proj stage writes x0 | x1 | v as before round 3
    h->no_pad_skip = debug_flag("no_pad_skip");        // tiles inside a read's [PAD] prefix are computed like any other
    h->row_h = debug_flag("row_h") || debug_flag("stamp");   // the fused 16-bit tail kernels keep h in row order inside every tile
                                                             // (the stamped developer build of the tail kernel exists in that form only)
    h->no_seg_skip = debug_flag("no_seg_skip");        // ... and segments inside it are transformed like any other (pad_prefix.hip, SegPrefix)
    h->cfg = *cfg;
    if (cfg->precision == CLM_PREC_F16X3) {             // an exact-fp32 engine whose fused tails multiply hi + lo halfs
        h->x3 = true;
        h->cfg.precision = CLM_PREC_F32;
        if (h->unfused_fp32) { delete h; return fail<clm_handle>(nullptr, CLM_E_UNSUPPORTED, "CLM_PREC_F16X3 exists in the fused tail kernels only (CLM_DEBUG=unfused_fp32 is set)"); }
    }
    h->device = device;
    if (hipHostMalloc((void**)&h->bad_ids, sizeof(int), hipHostMallocMapped) == hipSuccess) *h->bad_ids = 0;
    else h->bad_ids = nullptr;
    *out = h;
    return CLM_OK;
}

int clm_load_weight(clm_handle* h, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !key || !data || !shape || ndim < 1 || ndim > 4) return fail(h, CLM_E_INVALID, "clm_load_weight: bad argument");
    std::string ck;
    if (!canonical_key(key, ck)) return fail(h, CLM_E_INVALID, std::string("unknown weight key: ") + key);
    if (ck.find("implicit_filter.3.freq") != std::string::npos || ck.find("implicit_filter.5.freq") != std::string::npos)
        return CLM_OK;  // aliases of the shared sine module's parameter (implicit_filter.1.freq)
    const KeySpec* spec = nullptr;
    static thread_local std::vector<KeySpec> specs;
    specs = expected_keys(h);
    for (auto& s : specs)
        if (s.key == ck) spec = &s;
    if (!spec) return fail(h, CLM_E_INVALID, std::string("unknown weight key: ") + key);
    std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != spec->shape) {
        std::string got, want;
        for (auto v : shp) got += std::to_string(v) + ",";
        for (auto v : spec->shape) want += std::to_string(v) + ",";
        return fail(h, CLM_E_INVALID, std::string(key) + ": shape [" + got + "] does not match [" + want + "]");
    }
    size_t n = 1;
    for (auto v : shp) n *= (size_t)v;
    HIPCHK(h, hipSetDevice(h->device));
    Tensor& t = h->w[ck];
    if (!t.d) HIPCHK(h, t.d.alloc(n * 4));
    if (dtype == CLM_DT_F32) {
        HIPCHK(h, hipMemcpy(t.d.get(), data, n * 4, hipMemcpyDefault));
    } else if (dtype == CLM_DT_F64 || dtype == CLM_DT_BF16 || dtype == CLM_DT_F16) {
        size_t es = dtype == CLM_DT_F64 ? 8 : 2;
        DevBuf stage;
        HIPCHK(h, stage.alloc(n * es));
        HIPCHK(h, hipMemcpy(stage.get(), data, n * es, hipMemcpyDefault));
        hipLaunchKernelGGL(convert_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, stage.get(), t.d.get<float>(), n, dtype);
        HIPCHK(h, hipDeviceSynchronize());                    // (before `stage` is freed)
    } else {
        return fail(h, CLM_E_INVALID, "clm_load_weight: dtype must be f32/f64/bf16/f16");
    }
    t.loaded = true;
    h->finalized = false;
    return CLM_OK;
}

int clm_finalize(clm_handle* h) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    for (auto& s : expected_keys(h)) {                       // the pointers every later launch takes: blk / net / hw
        const auto it = h->w.find(s.key);
        if (it == h->w.end() || !it->second.loaded) return fail(h, CLM_E_MISSING, "missing weight: " + s.key);
        *s.dst = it->second.d.get<float>();
    }
    HIPCHK(h, hipDeviceSynchronize());
    h->rows.valid = false;
    ++h->rows.generation;
    h->filters.clear();                                      // (functions of the weights; each packing below replaces its own)
    h->pad_tables.clear();
    const int prec = h->cfg.precision;
    // hi + lo halfs of the tail weights: an fp16x3 handle's own arithmetic; a 16-bit handle's short reads and first fall-back level
    const bool pack_x3 = (h->x3 || prec != PREC_F32) && !h->unfused_fp32;
    h->x3_wmax = 0.f;
    hipStream_t st = 0;
    for (int i = 0; i <= NLAYER; ++i)              // the four tail products of every block, then (i == NLAYER) the score layer
        for (int j = 0; j < (i < NLAYER ? 4 : 1); ++j) {
            const float* src = i < NLAYER ? h->blk[i].w[j] : h->net.att_w1;
            const int n = i < NLAYER ? MAT_N[j] : D, k = i < NLAYER ? MAT_K[j] : D;
            // (fp16c: the two MLP products run on plain fp16 weights -- tail16_kernel, MLP_PREC -- or, second level, on hi + lo)
            const bool mlp16c = prec == PREC_F16C && i < NLAYER && j >= 2;
            int rc;
            if ((rc = pack_gemm(h, mlp16c ? (int)PREC_F16 : prec, src, n, k, h->pk_mode.slot(i, j), st))) return rc;
            if (mlp16c && (rc = pack_gemm(h, PREC_F16C, src, n, k, h->pk_mlpc.slot(i, j), st))) return rc;
            if (prec != PREC_F32 && (rc = pack_gemm(h, PREC_F32, src, n, k, h->pk_f32.slot(i, j), st))) return rc;
            if ((rc = pack_tail(h, false, src, n, k, h->pk_t32.slot(i, j), st))) return rc;
            if (!pack_x3) continue;
            if ((rc = pack_tail(h, true, src, n, k, h->pk_x3.slot(i, j), st))) return rc;
            float m = 0.f;                                   // what the hi + lo packing must hold
            HIPCHK(h, device_max_abs(src, (size_t)n * k, m));
            if (m != m || m > h->x3_wmax) h->x3_wmax = m;            // (NaN stays)
        }
    if (prec != PREC_F32)
        for (int i = 0; i < NLAYER; ++i) {
            HIPCHK(h, h->fir[i].alloc((size_t)D * 3 * sizeof(float4)));
            launch_fir_table(h->blk[i].short_w, h->blk[i].short_b, h->blk[i].b_in, h->fir[i].get<float4>(), st);
        }
    HIPCHK(h, h->ztab.alloc((size_t)VOCAB * D3 * 4));
    launch_ztab(h->net.emb, h->blk[0].ln1_g, h->blk[0].ln1_b, h->blk[0].w[0], h->blk[0].b_in, h->ztab.get<float>(), h->cfg.ln_eps, st);
    const struct { int rows, cols; const float** t; } tr[5] = {   // the classifier's matrices, transposed [in][out]
        {HH, D, &h->hw.w0t}, {HH, HH, &h->hw.w3t}, {HH, HH, &h->hw.w60t}, {HH, HH, &h->hw.w63t}, {NCLS, HH, &h->hw.wot}};
    for (int j = 0; j < 5; ++j) {
        HIPCHK(h, h->head_t[j].alloc((size_t)tr[j].rows * tr[j].cols * 4));
        launch_transpose(h->net.cls[j], h->head_t[j].get<float>(), tr[j].rows, tr[j].cols, st);
        *tr[j].t = h->head_t[j].get<float>();
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    return CLM_OK;
}

int clm_reserve(clm_handle* h, int B, int L) {
    if (!h || B < 1 || L < 1) return fail(h, CLM_E_INVALID, "clm_reserve: bad argument");
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_reserve before clm_finalize");
    HIPCHK(h, hipSetDevice(h->device));
    FilterSet* fs = nullptr;
    const ReversedFilter* kr = nullptr;
    if (int rc = ensure_filters(h, L, 0, &fs, &kr)) return rc;
    const int chunk = chunk_for(h, L);
    return ensure_workspace(h, plan_chunk(h, B < chunk ? B : chunk, L), 0);
}

int clm_forward_traj(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                     const clm_attn_out* attn, const clm_traj_out* traj, void* stream) {
    if (!h) return CLM_E_INVALID;
    const char* const who = traj ? "clm_forward_traj" : (attn ? "clm_forward_attn" : "clm_forward");
    if (!h->finalized) return fail(h, CLM_E_STATE, std::string(who) + " before clm_finalize");
    if (int rc = check_ids_arg(h, who, ids, logits_out, ids_dtype, ids_row_stride, B, L)) return rc;
    if (int rc = check_attn_arg(h, who, attn, L)) return rc;
    if (int rc = check_traj_arg(h, who, traj, L)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = check_bad_ids(h)) return rc;
    return forward_all(h, ids, ids_dtype, ids_row_stride, B, L, logits_out, reinterpret_cast<hipStream_t>(stream), attn, traj);
}

int clm_forward_attn(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, float* logits_out,
                     const clm_attn_out* attn, void* stream) {
    return clm_forward_traj(h, ids, ids_dtype, ids_row_stride, B, L, logits_out, attn, nullptr, stream);
}

int clm_forward(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L,
                float* logits_out, void* stream) {
    return clm_forward_attn(h, ids, ids_dtype, ids_row_stride, B, L, logits_out, nullptr, stream);
}

int clm_stage_ids(clm_handle* h, const void* host_ids, int ids_dtype, int64_t ids_row_stride, int B, int L, int* staged) {
    if (!h) return CLM_E_INVALID;
    if (int rc = check_ids_arg(h, "clm_stage_ids", host_ids, staged, ids_dtype, ids_row_stride, B, L)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    const int k = h->next_stage;
    clm_handle::Stage& s = h->stage[k];
    if (s.pending) return fail(h, CLM_E_STATE, "clm_stage_ids: both staging buffers hold batches not yet run (clm_forward_staged)");
    const size_t bytes = (size_t)B * (size_t)ids_row_stride * ids_elem_size(ids_dtype);
    if (!s.copied) {
        HIPCHK(h, hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming));
    }
    if (s.used) HIPCHK(h, hipStreamWaitEvent(h->copy_stream, s.consumed, 0));   // the forward that read this buffer is done
    if (bytes > s.buf.bytes()) {
        if (s.buf) HIPCHK(h, hipEventSynchronize(s.consumed));
        HIPCHK(h, s.buf.reserve(bytes));
    }
    HIPCHK(h, hipMemcpyAsync(s.buf.get(), host_ids, bytes, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipEventRecord(s.copied, h->copy_stream));
    s.dtype = ids_dtype; s.B = B; s.L = L; s.stride = ids_row_stride;
    s.pending = true;
    h->next_stage = k ^ 1;
    *staged = k;
    return CLM_OK;
}

int clm_forward_staged(clm_handle* h, int staged, float* logits_out, void* stream) {
    return clm_forward_staged_attn(h, staged, logits_out, nullptr, stream);
}

int clm_forward_staged_attn(clm_handle* h, int staged, float* logits_out, const clm_attn_out* attn, void* stream) {
    return clm_forward_staged_traj(h, staged, logits_out, attn, nullptr, stream);
}

int clm_forward_staged_traj(clm_handle* h, int staged, float* logits_out, const clm_attn_out* attn, const clm_traj_out* traj,
                            void* stream) {
    if (!h) return CLM_E_INVALID;
    if (staged < 0 || staged > 1 || !h->stage[staged].pending)
        return fail(h, CLM_E_STATE, "clm_forward_staged: no batch staged in that buffer");
    clm_handle::Stage& s = h->stage[staged];
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(h, hipStreamWaitEvent(st, s.copied, 0));
    const int rc = clm_forward_traj(h, s.buf.get(), s.dtype, s.stride, s.B, s.L, logits_out, attn, traj, stream);
    // whatever happened, the buffer is no longer "staged and waiting": a failed forward must not wedge it for good
    s.pending = false;
    s.used = true;
    (void)hipEventRecord(s.consumed, st);
    return rc;
}

int clm_stage_wait(clm_handle* h, int staged) {
    if (!h) return CLM_E_INVALID;
    if (staged < 0 || staged > 1 || !h->stage[staged].copied) return fail(h, CLM_E_STATE, "clm_stage_wait: nothing was staged there");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->stage[staged].copied));
    return check_bad_ids(h);
}

int clm_check(clm_handle* h, void* stream) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return check_bad_ids(h);
}

int clm_selfcheck(clm_handle* h, const void* ids, int ids_dtype, int64_t ids_row_stride, int B, int L, void* stream,
                  float* max_abs_diff, int* labels_differ) {
    if (!h) return CLM_E_INVALID;
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_selfcheck before clm_finalize");
    if (int rc = check_ids_arg(h, "clm_selfcheck", ids, max_abs_diff, ids_dtype, ids_row_stride, B, L)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    *max_abs_diff = 0.f;
    if (labels_differ) *labels_differ = 0;
    if (is_exact(h)) return CLM_OK;
    if (int rc = grow(h, Sync::Stream(st), {{&h->sc_logits, (size_t)2 * B * NCLS * 4}})) return rc;
    int rc = CLM_OK;
    {
        RunScope<clm_handle> scope(h);
        h->run.fallback = 0;                                    // the MODE is on trial (short reads of fp16c: its fp16x3 kernels)
        // pass 0: the arithmetic the handle's mode runs reads of this length in (whatever clm_set_fallback says); pass 1: exact fp32
        for (int pass = 0; pass < 2 && !rc; ++pass) {
            h->run.force_prec = pass == 0 ? mode_prec(h, L) : (int)PREC_F32;
            h->run.referee = pass == 1;
            rc = forward_all(h, ids, ids_dtype, ids_row_stride, B, L, h->sc_logits.get<float>() + (size_t)pass * B * NCLS, st);
        }
    }
    if (rc) return rc;
    return logits_deviation(h, st, h->sc_logits.get<float>(), B, max_abs_diff, labels_differ);
}

int clm_logit_deviation(const float* a, const float* b, int B, int n_classes, float* max_abs_diff, int* labels_differ) {
    if (!a || !b || !max_abs_diff || B < 0 || n_classes < 1) return CLM_E_INVALID;
    float worst = 0.f;
    int differ = 0;
    for (int r = 0; r < B; ++r) {
        const float *x = a + (size_t)r * n_classes, *y = b + (size_t)r * n_classes;
        int ax = 0, ay = 0;
        for (int c = 0; c < n_classes; ++c) {
            const float d = std::fabs(x[c] - y[c]);
            if (!(d <= 3.0e38f)) worst = INFINITY;             // NaN or inf anywhere = infinitely wrong, and it STAYS so
            else if (d > worst) worst = d;
            if (x[c] > x[ax]) ax = c;
            if (y[c] > y[ay]) ay = c;
        }
        differ += ax != ay;
    }
    *max_abs_diff = worst;
    if (labels_differ) *labels_differ = differ;
    return CLM_OK;
}

int clm_set_fallback(clm_handle* h, int on) {
    if (!h) return CLM_E_INVALID;
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_set_fallback before clm_finalize");
    if (on < 0 || on > 2) return fail(h, CLM_E_INVALID, "clm_set_fallback: level must be 0, 1 or 2");
    h->run.fallback = is_exact(h) ? 0 : on;                    // (an exact-fp32 handle has nothing to fall back to)
    return CLM_OK;
}

int clm_set_mlp_compensation(clm_handle* h, int on) {
    if (!h) return CLM_E_INVALID;
    if (h->cfg.precision != PREC_F16C) return fail(h, CLM_E_UNSUPPORTED, "clm_set_mlp_compensation: not a CLM_PREC_F16C handle");
    h->mlp_lo = on != 0;
    return CLM_OK;
}

int clm_set_short_read_len(clm_handle* h, int min_len) {
    if (!h || min_len < 1) return fail(h, CLM_E_INVALID, "clm_set_short_read_len: bad argument");
    if (h->cfg.precision != PREC_F16C) return fail(h, CLM_E_UNSUPPORTED, "clm_set_short_read_len: not a CLM_PREC_F16C handle");
    h->f16c_min_len = min_len;
    return CLM_OK;
}

int clm_effective_precision(const clm_handle* h, int L) {
    if (!h || L < 1) return CLM_E_INVALID;
    const ChunkPlan p = plan_chunk(h, 1, L);
    return p.x3 ? CLM_PREC_F16X3 : p.prec;
}

int clm_debug_stop_after(clm_handle* h, int layer, int stage) {
    if (!h) return CLM_E_INVALID;
    h->stop_layer = layer;
    h->stop_stage = stage;
    return CLM_OK;
}

int clm_debug_fetch(clm_handle* h, const char* name, void* host_out, size_t bytes) {
    if (!h || !name || !host_out) return fail(h, CLM_E_INVALID, "clm_debug_fetch: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const size_t es = plan_chunk(h, h->last_B, h->last_L).es;
    const size_t B = h->last_B, L = h->last_L, Lp = h->last_Lp;
    const void* src = nullptr;
    size_t have = 0;
    std::string n(name);
    if (n == "hidden" || n == "h") { src = h->h.get<float>(); have = B * L * D * 4; }
    else if (n == "z") { src = h->z.get(); have = B * D3 * Lp * es; }
    else if (n == "y") { src = h->y.get(); have = B * D * Lp * es; }
    else if (n == "u") { src = h->u.get(); have = B * L * DI * es; }
    else if (n == "scores") { src = h->scores.get<float>(); have = B * L * 4; }
    else if (n == "pooled") { src = h->pooled.get<float>(); have = B * D * 4; }
    else if (n.rfind("filter.", 0) == 0) {
        int i = std::atoi(n.c_str() + 7);
        const int key = conv_segments_for((int)L) > 1 ? KEY_LONG : conv_logn_for((int)L);
        for (auto& f : h->filters)          // the first L taps of the class's filter (they do not depend on L)
            if (f.key == key && i >= 0 && i < NLAYER && (int)L <= f.Lf) { src = f.ktime[i].get(); have = L * D * 4; }
    }
    if (!src) return fail(h, CLM_E_INVALID, "clm_debug_fetch: unknown or empty buffer " + n);
    if (int rc = fetch_bytes(h, "clm_debug_fetch", n, src, have, host_out, bytes)) return rc;
    if (src == h->h.get<float>() && h->last_hreg_Lmain > 0) {
        // the tail kernels left the whole tiles in register order (gemm16.hip HREG): [mt][q][thread][4 floats] inside each tile's
        // 128 KiB, thread = (wave, lhalf, lrow), value = token 32 mt + lrow, feature 32 wave + 8 q + 4 lhalf + j -- back to rows here
        constexpr size_t TILE = (size_t)128 * D;
        std::vector<float> blk(TILE);
        float* const out = static_cast<float*>(host_out);
        const size_t nf = bytes / 4;
        for (size_t b = 0; b < B; ++b)
            for (size_t t0 = 0; t0 + 128 <= (size_t)h->last_hreg_Lmain; t0 += 128) {
                const size_t base = (b * L + t0) * D;
                if (base >= nf) break;
                if (base + TILE <= nf) std::copy(out + base, out + base + TILE, blk.begin());
                else HIPCHK(h, hipMemcpy(blk.data(), h->h.get<float>() + base, TILE * 4, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < TILE && base + i < nf; ++i) {
                    const size_t t = i / D, f = i % D, mt = t / 32, lrow = t % 32, wave = f / 32, q = f % 32 / 8, lhalf = f % 8 / 4, j = f % 4;
                    out[base + i] = blk[((mt * 4 + q) * 512 + wave * 64 + lhalf * 32 + lrow) * 4 + j];
                }
            }
    }
    return CLM_OK;
}

// ---- the head fine-tune: residual rows out, attention pooling forward / backward on the caller's weights (pool_train.hip)
int clm_rows(clm_handle* h, const float** rows, int* B, int* L) {
    if (!h) return CLM_E_INVALID;
    if (!rows || !B || !L) return fail(h, CLM_E_INVALID, "clm_rows: bad argument");
    if (!h->finalized) return fail(h, CLM_E_STATE, "clm_rows before clm_finalize");
    if (!h->rows.valid) return fail(h, CLM_E_STATE, "clm_rows: no completed forward on this handle since its weights were loaded");
    if (!h->rows.one_chunk)
        return fail(h, CLM_E_STATE, "clm_rows: the last forward ran " + std::to_string(h->rows.B) + " reads in chunks of chunk_reads = " +
                                        std::to_string(h->cfg.chunk_reads) + "; only its last chunk's rows are left");
    if (!h->rows.exact)
        return fail(h, CLM_E_UNSUPPORTED, "clm_rows: the last forward ran 16-bit kernels; the rows are an output of the exact-fp32 and fp16x3 kernels only");
    *rows = h->h.get<float>();
    *B = h->rows.B;
    *L = h->rows.L;
    return CLM_OK;
}

int64_t clm_rows_generation(const clm_handle* h) { return h ? h->rows.generation : -1; }

int clm_chunk_reads(const clm_handle* h, int L) {
    if (!h || L < 1 || !h->finalized) return CLM_E_INVALID;
    return chunk_for(h, L);
}

namespace {
// the kernels read rows, weights and pooled vectors 16 bytes at a time
bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) % 16) return false;
    return true;
}
int check_pool_args(clm_handle* h, const char* who, bool any_null, bool aligned, int B, int L) {
    const std::string w(who);
    if (any_null || B < 1 || L < 1) return fail(h, CLM_E_INVALID, w + ": bad argument (a null pointer, or B or L < 1)");
    if (!aligned) return fail(h, CLM_E_INVALID, w + ": rows, the weights and the pooled vectors must be 16-byte aligned");
    if (!h->finalized) return fail(h, CLM_E_STATE, w + " before clm_finalize");
    if (B > 65535 || L > h->cfg.max_seq_len) return fail(h, CLM_E_UNSUPPORTED, w + ": at most 65535 reads of max_seq_len tokens");
    return CLM_OK;
}
// the call's workspace: W1 in the packing its kernels read, and the partials -- grown behind the stream's queued work
int pool_workspace(clm_handle* h, DevBuf& w1, size_t partial_bytes, hipStream_t st) {
    return grow(h, Sync::Stream(st), {{&w1, (size_t)D * D * 4}, {&h->pt_partial, partial_bytes}});
}
}  // namespace

int clm_pool_forward(clm_handle* h, const float* rows, int B, int L, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* scores_out, float* stats_out, float* pooled_out, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (int rc = check_pool_args(h, "clm_pool_forward", !rows || !w1 || !b1 || !w2 || !b2 || !scores_out || !stats_out || !pooled_out,
                                 aligned16({rows, w1, b1, w2, scores_out, pooled_out}), B, L)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = pool_workspace(h, h->pt_w1s, (size_t)B * POOL_SPLIT * 4 * D * 4, st)) return rc;
    const float eps = h->cfg.ln_eps;
    HIPCHK(h, hipMemsetAsync(h->pt_w1s.get(), 0, h->pt_w1s.bytes(), st));
    launch_pack_weight(PREC_F32, w1, h->pt_w1s.get(), D, D, st);
    launch_score(rows, h->net.lnf_g, h->net.lnf_b, h->pt_w1s.get(), b1, w2, b2, scores_out, B, L, eps, st);
    launch_softmax_stats(scores_out, stats_out, B, L, st);
    launch_pool(rows, h->net.lnf_g, h->net.lnf_b, scores_out, stats_out, h->pt_partial.get<float>(), B, L, eps, st);
    launch_pool_combine(h->pt_partial.get<float>(), pooled_out, B, st);
    return launched(h, "clm_pool_forward");
}

int clm_pool_backward(clm_handle* h, const float* rows, int B, int L, const float* w1, const float* b1, const float* w2,
                      const float* scores, const float* stats, const float* pooled, const float* dpooled, float* d_w1, float* d_b1,
                      float* d_w2, float* d_b2, float beta, void* stream) {
    if (!h) return CLM_E_INVALID;
    if (int rc = check_pool_args(h, "clm_pool_backward", !rows || !w1 || !b1 || !w2 || !scores || !stats || !pooled || !dpooled || !d_w1 ||
                                 !d_b1 || !d_w2 || !d_b2, aligned16({rows, w1, b1, w2, scores, pooled, dpooled}), B, L)) return rc;
    if (beta != 0.f && beta != 1.f) return fail(h, CLM_E_INVALID, "clm_pool_backward: beta must be 0 or 1");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = pool_workspace(h, h->pt_w1t, (size_t)pool_bwd_grid(B, L) * POOL_BWD_PSTRIDE * 4, st)) return rc;
    launch_pack_f32t(w1, h->pt_w1t.get(), D, D, st);
    launch_pool_bwd(rows, h->net.lnf_g, h->net.lnf_b, h->pt_w1t.get(), b1, w2, scores, stats, pooled, dpooled, h->pt_partial.get<float>(),
                    d_w1, d_b1, d_w2, d_b2, beta, B, L, h->cfg.ln_eps, st);
    return launched(h, "clm_pool_backward");
}

int clm_profile_enable(clm_handle* h, int on) {
    if (!h) return CLM_E_INVALID;
    h->run.prof = on != 0;
    return CLM_OK;
}

int clm_profile_read(clm_handle* h, double* ms_out, int64_t* launches_out, int reset) {
    if (!h) return CLM_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    h->profile.read(ms_out, launches_out, reset != 0);
    return CLM_OK;
}

const char* clm_profile_stage_name(int stage) {
    static const char* names[CLM_N_STAGES] = {"embed", "ln1_in_proj", "short_long_conv", "out_proj", "ln2_fc1_gelu",
                                              "fc2", "lnf_pool_score", "softmax_pool", "head_mlp", "filter",
                                              "out_proj_ln2_mlp", "ln2_mlp"};
    return (stage >= 0 && stage < CLM_N_STAGES) ? names[stage] : "?";
}

const char* clm_last_error(const clm_handle* h) { return h ? h->err.c_str() : create_error<clm_handle>().c_str(); }

int clm_destroy(clm_handle* h) {
    return destroy_handle(h, [h] {                           // (with the device idle: bad_ids is written by queued kernels)
        tail16_dump_stamps();
        conv_dump_stamps();
        for (auto& sg : h->stage) {
            if (sg.copied) (void)hipEventDestroy(sg.copied);
            if (sg.consumed) (void)hipEventDestroy(sg.consumed);
        }
        if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
        if (h->bad_ids) (void)hipHostFree(h->bad_ids);
    });
}

}  // extern "C"
