"""CPU error model of the 16-bit engine modes (developer tool; test infrastructure: it imports the oracle).

Runs the oracle's forward in float64 with selectable roundings to fp16 / bf16 / split (hi + lo) at exactly the places the
HIP path rounds: GEMM activation operands (LN1, y, LN2, GELU output, ln_f), packed weights, and the z / y tensors stored
between the tail kernel and the long convolution.  Prints the max |logit error| against the unrounded float64 forward for
each ablation, so that the cheapest set of compensations meeting north_star's 1e-3 can be chosen before any kernel is
written.       python tests/error_model.py [B L]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import torch.nn.functional as F

from oracle import hyena_oracle as ho

DT = torch.float64


def rnd(x, mode):
    """mode: None exact | 'h' fp16 | 'b' bf16 | 'hh' fp16 hi + fp16 lo | 'h8' fp16 + e4m3-grade lo (4 significant bits)
    | 'h5' fp16 + e5m2-grade lo (3 significant bits: the lo bytes of fp16c's activations, gemm_common.h lo8_pack4)"""
    if mode is None:
        return x
    if mode == "h":
        return x.to(torch.float16).to(DT)
    if mode == "b":
        return x.to(torch.bfloat16).to(DT)
    if mode == "hh":
        hi = x.to(torch.float16).to(DT)
        return hi + (x - hi).to(torch.float16).to(DT)
    if mode == "h8":
        hi = x.to(torch.float16).to(DT)
        lo = x - hi
        m, e = torch.frexp(lo)
        return hi + torch.ldexp(torch.round(m * 16) / 16, e)
    if mode == "h5":
        hi = x.to(torch.float16).to(DT)
        m, e = torch.frexp(x - hi)
        return hi + torch.ldexp(torch.round(m * 8) / 8, e)
    raise ValueError(mode)


def lin(x, sd, key, am, wm, peel=False):
    """peel: the last token's row takes the product of the unrounded operands (the fp32 matrix-vector chain of lone_token.hip)"""
    if isinstance(wm, dict):
        wm = next((v for k, v in wm.items() if k in key), None)
    b = sd.get(key + ".bias")
    b = None if b is None else b.to(DT)
    out = F.linear(rnd(x, am), rnd(sd[key + ".weight"].to(DT), wm), b)
    if peel:
        out[:, -1] = F.linear(x[:, -1], sd[key + ".weight"].to(DT), b)
    return out


def forward(ids, sd, cfg, trace=None):
    """cfg keys: a_ln1, a_y, a_ln2, a_gelu, a_lnf (activation operand modes), w (weights), z, y (storage), pool (pooled
    vector taken from the rounded ln_f tile); zg: z is stored behind the short filter and the gate (x0f and g = x1f * vf, the gated
    hand-over of gemm16.hip inproj_blocks_gated) instead of in front of them; peel: reads of 128 k + 1 > 128 tokens run their last
    token through unrounded products (clm_api.hip plan_chunk, p.peel) -- its y and z are still stored rounded.
    trace: a dict that receives every block's residual rows `l{i}.out` [B, L, 256] (l3.out: the rows in front of ln_f) and the
    pooling `scores` [B, L]"""
    g = cfg.get
    ids = torch.as_tensor(ids, dtype=torch.int64)
    h = F.embedding(ids, sd[ho.BB + "embeddings.word_embeddings.weight"].to(DT))
    L = h.shape[1]
    pl = bool(g("peel")) and L > 128 and L % 128 == 1
    for i in range(ho.N_LAYER):
        p = f"{ho.BB}layers.{i}."
        u = ho._ln(h, sd, p + "norm1", DT)
        if i == 0 and g("block0_exact", True):       # the engine looks block 0's in_proj up in an fp32 table by token id
            z = lin(u, sd, p + "mixer.in_proj", None, None).transpose(1, 2)
            zmode = None
        else:
            z = lin(u, sd, p + "mixer.in_proj", g("a_ln1"), g("w"), pl).transpose(1, 2)
            zmode = g("z")
        if g("zg"):
            x0, x1, v = ho.short_filter(z, sd, i, DT).split(ho.D_MODEL, dim=1)
            x0, gate = rnd(x0, zmode), rnd(v * x1, zmode)
        else:
            x0, x1, v = ho.short_filter(rnd(z, zmode), sd, i, DT).split(ho.D_MODEL, dim=1)
            gate = v * x1
        k = ho.hyena_filter(sd, i, L, DT).transpose(0, 1)
        v = ho.fftconv(gate, k, sd[p + "mixer.filter_fn.bias"].to(DT))
        y = rnd(v * x0, g("y"))
        r = lin(rnd(y.transpose(1, 2), g("a_y")), sd, p + "mixer.out_proj", None, g("w"), pl) + h
        m = lin(ho._ln(r, sd, p + "norm2", DT), sd, p + "mlp.fc1", g("a_ln2"), g("w"), pl)
        h = lin(F.gelu(m, approximate="tanh"), sd, p + "mlp.fc2", g("a_gelu"), g("w"), pl) + r
        if trace is not None:
            trace[f"l{i}.out"] = h
    hid = ho._ln(h, sd, ho.BB + "ln_f", DT)
    s = ho._lin(F.gelu(lin(hid, sd, ho.HD + "attention.0", g("a_lnf"), g("w"), pl)), sd, ho.HD + "attention.2", DT)
    if trace is not None:
        trace["scores"] = s[..., 0]
    a = torch.softmax(s, dim=1)
    pooled = (rnd(hid, g("pool")) * a).sum(dim=1)
    x = F.gelu(ho._lin(pooled, sd, ho.HD + "classifier.0", DT))
    x = F.gelu(ho._lin(x, sd, ho.HD + "classifier.3", DT))
    x = ho._lin(F.gelu(ho._lin(x, sd, ho.HD + "classifier.6.layers.0", DT)), sd, ho.HD + "classifier.6.layers.3", DT) + x
    return ho._lin(x, sd, ho.HD + "output_layer", DT)


ACT = ("a_ln1", "a_y", "a_ln2", "a_gelu", "a_lnf")
ALL16 = {**{k: "h" for k in ACT}, "w": "h", "z": "h", "y": "h", "pool": "h"}

# The engine's 16-bit modes as they run without a debug switch (clm_api.hip plan_chunk: fused tails, id-table block 0, the gated
# hand-over, the peeled last token).  fp16 / bf16: every GEMM operand, the packed weights and the stored z / y in the mode's type.
# fp16c (gemm_common.h, gemm16_common.h): in_proj / out_proj / attention.0 on fp16 hi + e4m3 lo weights; fc1 / fc2 on plain fp16
# weights (first level; clm_set_mlp_compensation is not modelled); the LayerNorm-1 and ln_f tiles, y and the gated rows of z as
# fp16 hi + one e5m2 lo byte; LayerNorm-2 and GELU tiles plain fp16.  Not modelled: the byte truncation of the hi operand inside the
# two lo products (5 % of a 2^-11 term), the fp32 arithmetic of the kernels themselves (two orders below a 16-bit rounding).
_W16C = {"in_proj": "h8", "out_proj": "h8", "attention": "h8", "fc1": "h", "fc2": "h"}
ENGINE_MODES = {
    "fp16": {**ALL16, "zg": True, "peel": True},
    "bf16": {**{k: "b" for k in ACT}, "w": "b", "z": "b", "y": "b", "pool": "b", "zg": True, "peel": True},
    "fp16c": {"a_ln1": "h5", "a_y": "h5", "a_lnf": "h5", "a_ln2": "h", "a_gelu": "h", "w": _W16C, "z": "h5", "y": "h5", "pool": None,
              "zg": True, "peel": True},
}


def main():
    B, L = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (6, 1000)
    wseed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    sd = ho.make_state_dict(wseed, head_scale=3.0)
    rows = []
    for seed in (99, 7):
        ids, _ = ho.synthetic_batch(5, B, L - 1, seed=seed)
        with torch.no_grad():
            ref = forward(ids, sd, {})
            W = lambda **kw: {"in_proj": "h", "out_proj": "h", "fc1": "h", "fc2": "h", "attention": "h", **kw}
            cases = {
                "all fp16 (the r01 fp16 mode)": ALL16,
                "P: all weights split": {**ALL16, "w": "hh"},
                "Q: in/out/att weights split": {**ALL16, "w": W(in_proj="hh", out_proj="hh", attention="hh")},
                "Q2: in/out weights split": {**ALL16, "w": W(in_proj="hh", out_proj="hh")},
                "R: Q + a_ln1 split": {**ALL16, "a_ln1": "hh", "w": W(in_proj="hh", out_proj="hh", attention="hh")},
                "S: R + a_lnf split + pool exact": {**ALL16, "a_ln1": "hh", "a_lnf": "hh", "pool": None, "w": W(in_proj="hh", out_proj="hh", attention="hh")},
                "T: S + y split (storage + operand)": {**ALL16, "a_ln1": "hh", "a_lnf": "hh", "pool": None, "y": "hh", "a_y": "hh", "w": W(in_proj="hh", out_proj="hh", attention="hh")},
                "U: T + fc1/fc2 weights split": {**ALL16, "a_ln1": "hh", "a_lnf": "hh", "pool": None, "y": "hh", "a_y": "hh", "w": "hh"},
                "V: U + z split": {**ALL16, "a_ln1": "hh", "a_lnf": "hh", "pool": None, "y": "hh", "a_y": "hh", "z": "hh", "w": "hh"},
                "P2: all weights split + pool exact": {**ALL16, "w": "hh", "pool": None},
                "P3: P2 + a_ln1 split": {**ALL16, "w": "hh", "pool": None, "a_ln1": "hh"},
                "P4: P3 + a_lnf split": {**ALL16, "w": "hh", "pool": None, "a_ln1": "hh", "a_lnf": "hh"},
                "x3: everything split": {**{k: "hh" for k in ACT}, "w": "hh", "y": "hh", "z": "hh"},
                "h8: everything fp16 + 4-bit lo": {**{k: "h8" for k in ACT}, "w": "h8", "y": "h8", "z": "h8"},
            }
            for name, cfg in cases.items():
                err = (forward(ids, sd, cfg) - ref).abs().max().item()
                rows.append((seed, name, err))
                print(f"seed {seed}  {B} x {L}  {name:44s} max |dlogit| {err:.2e}   (max |logit| {ref.abs().max():.2f})", flush=True)


def rank(L=2048, B=16, wseeds=(4, 6, 7, 1)):
    """`python tests/error_model.py rank [L B]`: rms / max logit error over B reads of the compensated-weights mode with ONE more
    operand (or a set) carried as hi + lo -- which activation rounding would be worth a lo term?  (Round 3: none alone; the error is
    spread over LN1, y, z and ln_f: -10 % each, -35..-45 % for LN1 + y together, -50..-65 % with z as well.  A max over a few reads
    is too noisy to rank by: removing one source can raise it.)"""
    stat = lambda e: f"rms {e.pow(2).mean().sqrt().item():.2e} max {e.abs().max().item():.2e}"
    for wseed in wseeds:
        sd = ho.make_state_dict(wseed, head_scale=3.0)
        ids, _ = ho.synthetic_batch(5, B, L - 1, seed=99 + wseed)
        with torch.no_grad():
            ref = forward(ids, sd, {})
            base = {**ALL16, "w": "hh"}
            cases = {"base (all 16-bit, weights hi + lo)": base, "LN1 hi + lo": {**base, "a_ln1": "hh"},
                     "y hi + lo": {**base, "y": "hh", "a_y": "hh"}, "z hi + lo": {**base, "z": "hh"},
                     "ln_f hi + lo, pool exact": {**base, "a_lnf": "hh", "pool": None},
                     "LN1 + y": {**base, "a_ln1": "hh", "y": "hh", "a_y": "hh"},
                     "LN1 + y + z": {**base, "a_ln1": "hh", "y": "hh", "a_y": "hh", "z": "hh"}}
            for n, c in cases.items():
                print(f"weights {wseed}  {B} x {L}  {n:36s} {stat(forward(ids, sd, c) - ref)}", flush=True)


# ------------------------------------------------------------------------------------------------------------- fp16x3 (AR_X3)
# The split of csrc/mfma32_common.h, operand by operand: hi = fp16(clamp(v)), lo = fp16(clamp(v - hi)) (split4; fp16's subnormals
# kept), weights x 2^10 (pack_x3_kernel), the three products w_hi a_hi + w_lo a_hi + w_hi a_lo, accumulated in float64 -- so what is
# left is the error of the FORMAT: an activation below ~2^-3 has its lo half in fp16's subnormal range (an absolute 2^-25 instead of
# a relative 2^-22).  `flush`: fp16 subnormal halfs read as zero, what a matrix unit that flushes them would compute.
X3_WS = 1024.0
H_MAX, H_MIN_NORMAL = 65504.0, 2.0 ** -14


def x3_split(v: torch.Tensor, flush: bool = False):
    """(hi, lo) of v as float64 tensors holding fp16 values."""
    v = v.double()
    h16 = lambda t: t.clamp(-H_MAX, H_MAX).to(torch.float16).double()   # noqa: E731
    hi = h16(v)
    lo = h16(v - hi)
    if flush:
        hi = torch.where(hi.abs() < H_MIN_NORMAL, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < H_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def x3_linear(a: torch.Tensor, w: torch.Tensor, flush: bool = False) -> torch.Tensor:
    """a [..., K] @ w [N, K]^T in the fp16x3 format (float64 result)."""
    ah, al = x3_split(a, flush)
    wh, wl = x3_split(w.double() * X3_WS, flush)
    return (ah @ (wh + wl).T + al @ wh.T) / X3_WS


def mamba_x3_forward(variant: str, sd: dict, ids, mask=None, flush: bool = False, exact: bool = False, trace: dict | None = None):
    """Logits of a Mamba net (tests/mamba_stage_reference.py's stages in float64) with the three fp16x3 products of csrc/mamba.hip --
    the `mamba` front Linear, in_proj, out_proj with norm.weight folded in -- in the split format; `exact`: plain float64 products
    (the reference the split error is measured against).  `trace` receives the residual rows entering layer 0 ("front")."""
    import mamba_stage_reference as S

    lin = (lambda a, w: a @ w.T) if exact else (lambda a, w: x3_linear(a, w, flush))
    w = {k: v.detach().double() for k, v in sd.items()}
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    m = None if mask is None or variant != "mamba" else torch.as_tensor(np.asarray(mask), dtype=DT)
    pre = S.front_pre(variant, w, ids)
    h = S.front_post(variant, w, lin(pre, w["input_block.0.weight"]) if variant == "mamba" else None, pre, m)
    if trace is not None:
        trace["front"] = h
    for i in range(S.n_layers_of(sd)):
        p = S.layer_params(variant, sd, i, DT)
        zx = S.in_proj_post(p, lin(h, p["in_proj.weight"]))
        g, ssq = S.scan(p, zx, S.conv(p, zx))
        h = S.out_proj_post(p, h, lin(g, S.out_weight(p)), ssq, m)
    return S.head(w, S.pooled_of(S.partials(h), ids.shape[1]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rank":
        rank(*(int(a) for a in sys.argv[2:4]))
    else:
        main()
