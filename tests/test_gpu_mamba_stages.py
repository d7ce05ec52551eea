"""GPU (MI355X): every kernel of the Mamba INFERENCE path (csrc/mamba.hip) against float64, stage by stage and TOKEN BY TOKEN.

`predict` and `eval.py` run these kernels for model=mamba|mambasp, and tests/test_gpu_mamba.py judges them through two logits behind a
(mean + max) / 2 pooling over the whole read, which averages an error confined to one token, one head or one chunk boundary down by L.
Here every case is ONE forward of a one- or two-layer net (the production nets run exactly these kernel instances in every layer), after
which the workspace is fetched (`clm_mamba_debug_fetch`: "front", "layer0", "zx", "xc", "g", "ssq", "part", "pooled") and every stage is
compared, every token of it, with tests/mamba_stage_reference.py evaluated in float64 on the engine's OWN fetched input of that stage:
    front (mamba: Linear + LayerNorm + mask; mambasp: bit-equal to the embedding rows) -> in_proj (z | x | B | C per row; the dt columns per
    element, relative; the zero padding exactly 0) -> conv -> scan (g and ssq per token and head) -> out_proj (RMS scale, residual, mask)
    -> the 64-row pooling partials (maxima: exact selections of the rows) -> pooled.
A one-layer net shows all of it (its EPI_OUTPOOL stores the rows); the two-layer `mamba` shows the front, layer 0 as a whole through
EPI_OUT ("layer0"), layer 1's stages, and the masked partials as layer 1's only output (a fully masked tile: sums 0, maxima 0).

STATISTIC.  Per token: max_c |got - ref| / max_c |ref|, the token's own row maximum as denominator (g, ssq: the numerator per head; dt:
per element; part: per tile and channel over the sum of |rows| resp. max |rows|; a zero denominator demands an exact result).  Per read,
the max and the rms over tokens.  BOUND: engine <= max(K x the same statistic of the yardstick, 32 x 2^-24).  The yardstick is the same
stage in float32 on the CPU on the same input.  fp16x3 claims fp32 class: it gets the same yardstick and the same K on conv and scan
(exact fp32 in both precisions, and bit-equal between them on equal inputs: test_conv_and_scan_are_one_code_in_both_precisions) and,
at unit scale, on the projections.  In the activation-scale sweep the fp16x3 projections take the split model of the format as their
yardstick (tests/error_model.py x3_linear), with K_SPLIT.  No token is left out of any comparison.

SHAPES.  mambasp, one layer, d 256, B = 3 (read 0 left-padded by 17, read 1 by 0: the conv's first three tokens of reads 1 and 2 sit
right behind another read's rows), (expand, N) = (1, 16) the N < 32 zero padding | (2, 64) | (1, 128) the instance with addresses in
scratch | (3, 32) 12 heads, in_proj's n_real skip, each at L = 1, 63, 64, 65, 129 (the state carried twice), 200; d 512 (3, 128) at 200;
(3, 32) at 1,031.  mamba, two layers, (2, 64), 2 x 130, scattered masked tokens and a fully masked last tile.  Decay regimes at (1, 128),
2 x 200 (mamba_stage_reference.regime_state_dict; tests/test_mamba_stage_host.py holds the float32 yardstick below 1e-3 in each): flat
(dt 2e-4 ... 4e-4, A = 1), steep (dt 0.3 ... 0.8, A = 16: exp(s_63) underflows), mixed (in_proj's dt rows x 8: dt from 1e-8 to 11,
jumping by up to 1e9 between neighbours).  Activation scale at (2, 64), 3 x 200: embedding.weight x 2^0, 2^-4, 2^-8, 2^-12, 2^-16, and
the z rows of in_proj x 2^-8 (a small g under a residual stream that is not).

K, from the first run (no bound set before it).  Worst engine / yardstick ratio anywhere: 4.49 against the float32 yardstick (ssq of
one-token reads, both far below the floor; 3.31 among figures above the floor) -> K = 16, the smallest power of two >= 2 x 4.49 and
the cap.  3.86 against the split model (in_proj at unit scale: the model accumulates in fp64, the kernel in fp32; 1.01 among figures
above the floor) -> K_SPLIT = 8.  No ratio exceeded 8, so none needed an explanation from the code.

MEASURED on the MI355X, this tree (CLM_MAMBA_STAGE_PARITY=<file> appends every line; profiles/mamba_stage_parity.txt is one): the worst
engine / yardstick ratio over cases, reads and both statistics, with that case's largest per-token errors.
  float32 yardstick
    precision stage     worst ratio  engine max   yardstick  case
    fp32      front            1.35    7.66e-07    6.25e-07  mamba-2layers-e2-N64-L130-masked
    fp32      layer0           1.88    5.46e-07    3.23e-07  mamba-2layers-e2-N64-L130-masked
    fp32      in_proj          3.53    7.23e-07    2.41e-07  sp-e3-N32-L1
    fp32      dt               4.07    9.90e-07    4.07e-07  sp-e2-N64-L1
    fp32      conv             1.47    8.68e-08    8.68e-08  sp-e1-N128-L1
    fp32      g                3.92    5.87e-07    2.22e-07  sp-e3-N32-L200
    fp32      ssq              4.49    1.25e-07    1.64e-07  sp-e1-N128-L1
    fp32      out_proj         4.29    8.92e-07    2.08e-07  sp-e3-N32-L1
    fp32      part             2.14    2.52e-06    1.37e-06  mamba-2layers-e2-N64-L130-masked
    fp32      pooled           1.00    5.18e-08    5.18e-08  sp-e1-N16-L63
    fp16x3    front            0.93    5.07e-07    6.25e-07  mamba-2layers-e2-N64-L130-masked
    fp16x3    layer0           1.18    3.59e-07    4.04e-07  mamba-2layers-e2-N64-L130-masked
    fp16x3    in_proj          1.98    3.50e-07    2.10e-07  sp-e2-N64-L1
    fp16x3    dt               2.30    5.28e-07    4.07e-07  sp-e2-N64-L1
    fp16x3    conv             1.43    2.18e-07    1.79e-07  sp-e2-N64-L200
    fp16x3    g                3.93    5.67e-07    1.85e-07  sp-e3-N32-L200
    fp16x3    ssq              2.15    8.19e-07    5.76e-07  sp-e1-N128-L129
    fp16x3    out_proj         2.48    7.03e-07    3.76e-07  sp-e3-N32-L129
    fp16x3    part             2.44    3.30e-06    1.35e-06  mamba-2layers-e2-N64-L130-masked
    fp16x3    pooled           1.00    3.66e-08    3.66e-08  sp-e1-N16-L63
  split-model yardstick (fp16x3 projections of the scale sweep)
    precision stage     worst ratio  engine max   yardstick  case
    fp16x3    in_proj          3.86    3.81e-07    9.87e-08  scale-z2^-8
    fp16x3    dt               1.91    5.52e-07    2.89e-07  scale-E2^-4
    fp16x3    out_proj         3.31    5.08e-07    1.54e-07  scale-E2^-0

fp16x3's activation range (what the sweep prints; rms over tokens of the split model / the float32 product on the same input):
    in_proj   median |h| 6.8e-01: 0.3    4.3e-02: 1.1    2.7e-03: 15     1.7e-04: 240      1.0e-05: 3,800
    out_proj  median |g| 3.9e-02: 0.3    1.5e-03: 12     9.7e-05: 200    6.1e-06: 3,200    3.8e-07: 48,000 (a row off by 2.8 % of its maximum)
The kernels do what the format says (above the floor, engine / model = 1.00-1.02 at every scale: the MFMA keeps fp16 subnormals), and the
format leaves fp32 class below |v| ~ 4e-2.  The logits hide it behind the pooling: tests/test_gpu_mamba.py::test_small_activations
measures 1.6e-5 (x 2^-8) and 4.5e-5 (x 2^-16) relative to max(1, max |logit|) for fp16x3, inside the module's 1e-4, so no kernel changed.

SANITY of these tests, done once by hand on wrong-on-purpose builds: the conv reading the previous read's rows (its `tt >= 0` guard
replaced by a buffer-start guard) fails "conv" in 60 cases; the carried state without its exp(s_63) factor fails "g" in every case
of 129 tokens or more and in none below (a state carried once starts from zero); the N = 16 scan without its zeroed padding columns
fails every (1, 16) case (a non-finite g).  All three are gross enough that the logit tests of tests/test_gpu_mamba.py fail too.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import error_model as em
import mamba_reference as mr
import mamba_stage_reference as S
from mamba_stage_reference import REGIMES, regime_state_dict

pytestmark = pytest.mark.gpu

K = 16                      # x the float32 yardstick (exact fp32 everywhere; fp16x3 on conv, scan and, at unit scale, the projections)
K_SPLIT = 8                 # x the split-model yardstick (fp16x3 projections of the activation-scale sweep)
PAD = mr.PAD
PRECS = ("fp32", "fp16x3")
DEV = "cuda"                # where the float64 references run


# ------------------------------------------------------------------------------------------------------------- cases
def _sp_ids(seed, B, L):
    """Read 0 left-padded by 17, read 1 by 0, the others by 3: the first tokens of reads 1 and 2 sit right behind another read's rows."""
    ids = mr.synthetic_ids(seed, B, L)
    ids[0, :min(17, L - 1)] = PAD
    ids[2:, :min(3, L - 1)] = PAD
    return ids


def _sp_case(expand, N, L, d=256, B=3, seed=50):
    def make():
        sd = mr.make_mamba_state_dict("mambasp", seed, n_layers=1, d_model=d, expand=expand, d_state=N)
        return "mambasp", sd, _sp_ids(5000 + L, B, L), None
    return make


def _mamba_case():
    sd = mr.make_mamba_state_dict("mamba", 51, n_layers=2, d_model=256, expand=2, d_state=64, model_max_length=256)
    ids = mr.synthetic_ids(5100, 2, 130, pads=5)
    mask = (np.random.default_rng(5101).random((2, 130)) > 0.15).astype(np.float32)
    mask[1, 128:] = 0.0                                       # the whole last 64-row tile of read 1
    mask[0, 0] = mask[0, 64] = 0.0
    return "mamba", sd, ids, mask


def _regime_case(regime):
    def make():
        return "mambasp", regime_state_dict(regime), _sp_ids(5200, 2, 200), None
    return make


def _scale_case(k, zk=0):
    """(2, 64), L = 200, with embedding.weight x 2^-k and the z rows of in_proj x 2^-zk (a small g under a residual stream that is not)."""
    def make():
        sd = mr.make_mamba_state_dict("mambasp", 50, n_layers=1, d_model=256, expand=2, d_state=64)
        sd["embedding.weight"] = sd["embedding.weight"] * 2.0 ** -k
        W = sd["mamba_layers.0.in_proj.weight"].clone()
        W[:512] *= 2.0 ** -zk
        sd["mamba_layers.0.in_proj.weight"] = W
        return "mambasp", sd, _sp_ids(5200, 3, 200), None
    return make


PAIRS = [(1, 16), (2, 64), (1, 128), (3, 32)]
LENGTHS = [1, 63, 64, 65, 129, 200]
CASES = {f"sp-e{e}-N{n}-L{L}": _sp_case(e, n, L) for (e, n) in PAIRS for L in LENGTHS}
CASES["sp-d512-e3-N128-L200"] = _sp_case(3, 128, 200, d=512)
CASES["sp-e3-N32-L1031"] = _sp_case(3, 32, 1031)
CASES["mamba-2layers-e2-N64-L130-masked"] = _mamba_case
CASES.update({f"regime-{r}": _regime_case(r) for r in REGIMES})
SCALES = {f"scale-E2^-{k}": _scale_case(k) for k in (0, 4, 8, 12, 16)}
SCALES["scale-z2^-8"] = _scale_case(0, 8)


def _net(variant, sd, prec):
    from chimeralm_amd import mamba

    p = S.layer_params(variant, sd, 0, torch.float32)
    D = S.dims_of(p)
    kw = dict(vocab_size=12, embedding_dim=D.d, number_of_layers=S.n_layers_of(sd), number_of_classes=2, dropout=0.1,
              d_state=D.N, expand=D.di // D.d, precision=prec)
    if variant == "mamba":
        net = mamba.MambaSequenceClassification(model_max_length=sd["pos_embedding"].shape[1], **kw)
    else:
        net = mamba.MambaSequenceClassificationSP(**kw)
    net.load_state_dict(sd, strict=True)
    return net, D


def _forward(make, prec):
    """One forward; every tap as a float32 CPU tensor."""
    variant, sd, ids, mask = make()
    net, D = _net(variant, sd, prec)
    B, L = ids.shape
    logits = net(torch.from_numpy(ids).cuda(), None if mask is None else torch.from_numpy(mask).cuda()).cpu()
    assert net.precision_report.get("nonfinite_reruns", 0) == 0 and net.precision_report["fallback"] is False
    shapes = {"front": (B, L, D.d), "layer0": (B, L, D.d), "zx": (B, L, D.n_in_pad), "xc": (B, L, D.conv_dim), "g": (B, L, D.di),
              "ssq": (B, L, D.H), "part": (B, (L + 63) // 64, 2, D.d), "pooled": (B, D.d)}
    taps = {k: torch.from_numpy(net.debug_fetch(k, s)) for k, s in shapes.items()}
    taps["logits"] = logits
    net.close()
    return variant, sd, ids, mask, D, taps


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_MAMBA_STAGE_PARITY"):
        with open(os.environ["CLM_MAMBA_STAGE_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _stages(tag, prec, variant, sd, ids, mask, D, t, split=False):
    """Every stage of the forward that left the taps `t`: (stage, engine statistic, yardstick statistic, entries per token, K).
    The float64 reference runs on the device, the float32 yardstick on the CPU, both on the ENGINE's fetched input of the stage.
    `split`: the fp16x3 projections take the split model (error_model.x3_linear) as their yardstick."""
    dev = DEV
    nl = S.n_layers_of(sd)
    last = nl - 1
    B, L = ids.shape
    w64 = {k: v.detach().to(dev, torch.float64) for k, v in sd.items()}
    w32 = {k: v.detach().float() for k, v in sd.items()}
    idt = torch.from_numpy(ids)
    m32 = None if mask is None or variant != "mamba" else torch.from_numpy(mask)
    m64 = None if m32 is None else m32.to(dev, torch.float64)
    up = lambda x: x.to(dev, torch.float64)                    # noqa: E731
    use_split = split and prec == "fp16x3"
    kp = K_SPLIT if use_split else K
    out = []

    def add(stage, got, ref, yard, k=K, per=1, **kw):
        den = kw.pop("den", None)
        out.append((stage, S.statistic(up(got), ref, den=den, **kw), S.statistic(up(yard), ref, den=den, **kw), per, k))

    # ---- front
    if variant == "mambasp":
        assert torch.equal(t["front"], torch.nn.functional.embedding(idt, w32["embedding.weight"])), "front: not the embedding's rows"
    else:
        pre32 = S.front_pre(variant, w32, idt)
        y_yard = em.x3_linear(pre32, w32["input_block.0.weight"]).float() if use_split else None
        add("front", t["front"], S.front(variant, w64, idt.to(dev), m64), S.front_post(variant, w32, y_yard, pre32, m32), kp)
    # ---- layer 0 as a whole, where it is not the last (its workspace is gone): EPI_OUT's residual and mask through "layer0"
    if nl > 1:
        p64, p32 = S.layer_params(variant, sd, 0, torch.float64, dev), S.layer_params(variant, sd, 0, torch.float32)
        add("layer0", t["layer0"], S.layer(p64, up(t["front"]), m64), S.layer(p32, t["front"], m32))
    # ---- the last layer, stage by stage
    p64, p32 = S.layer_params(variant, sd, last, torch.float64, dev), S.layer_params(variant, sd, last, torch.float32)
    h_in = t["front"] if last == 0 else t["layer0"]
    zx = t["zx"][..., :D.n_in]
    assert not bool(t["zx"][..., D.n_in:].ne(0).any()), "in_proj: padding columns not exactly zero"
    zx64 = S.in_proj(p64, up(h_in))
    zx_y = S.in_proj_post(p32, em.x3_linear(h_in, p32["in_proj.weight"]).float()) if use_split else S.in_proj(p32, h_in)
    add("in_proj", zx[..., :D.dt0], zx64[..., :D.dt0], zx_y[..., :D.dt0], kp)
    add("dt", zx[..., D.dt0:], zx64[..., D.dt0:], zx_y[..., D.dt0:], kp, per=D.H, kind="element")
    add("conv", t["xc"], S.conv(p64, up(zx)), S.conv(p32, zx))
    g64, q64 = S.scan(p64, up(zx), up(t["xc"]))
    g32, q32 = S.scan(p32, zx, t["xc"])
    assert bool(torch.isfinite(t["g"]).all()) and bool(torch.isfinite(t["ssq"]).all()), "scan: non-finite output"
    add("g", t["g"], g64, g32, per=D.H, groups=D.H)
    add("ssq", t["ssq"], q64, q32, per=D.H, groups=D.H)
    rows64 = S.out_proj(p64, up(h_in), up(t["g"]), up(t["ssq"]), m64)
    if use_split:
        rows_y = S.out_proj_post(p32, h_in, em.x3_linear(t["g"], S.out_weight(p32)).float(), t["ssq"], m32)
    else:
        rows_y = S.out_proj(p32, h_in, t["g"], t["ssq"], m32)
    if last == 0:
        # a one-layer net stores the rows of EPI_OUTPOOL: out_proj by itself, then the pooling of the engine's own rows
        add("out_proj", t["layer0"], rows64, rows_y, kp)
        rows_e = up(t["layer0"])
        assert torch.equal(t["part"][:, :, 1], S.partials(t["layer0"])[:, :, 1]), "part: maxima are not selections of the rows"
        add("part", t["part"].reshape(B, -1, 1), S.partials(rows_e).reshape(B, -1, 1), S.partials(t["layer0"]).reshape(B, -1, 1),
            per=2 * D.d, kind="den", den=S.partial_scales(rows_e).reshape(B, -1, 1))
    else:
        add("part", t["part"].reshape(B, -1, 1), S.partials(rows64).reshape(B, -1, 1), S.partials(rows_y).reshape(B, -1, 1), kp,
            per=2 * D.d, kind="den", den=S.partial_scales(rows64).reshape(B, -1, 1))
    part64 = up(t["part"])
    add("pooled", t["pooled"][:, None], S.pooled_of(part64, L)[:, None], S.pooled_of(t["part"], L)[:, None])
    return out


def _hold(tag, prec, stages):
    rows, bad, summary = [], [], []
    for stage, e, y, per, k in stages:
        worst = S.check(f"{tag} {prec}", stage, e, y, k, rows, bad, per)
        summary.append(f"STAGE {tag:36s} {prec:6s} {stage:9s} engine max {float(e.max()):.2e} rms {float(e.pow(2).mean().sqrt()):.2e}  "
                       f"yardstick max {float(y.max()):.2e} rms {float(y.pow(2).mean().sqrt()):.2e}  K {k:2d}  worst ratio {worst:6.2f}")
    print("\n".join(rows))
    _record(summary)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_every_token(built_lib, name, prec):
    variant, sd, ids, mask, D, t = _forward(CASES[name], prec)
    if mask is not None:
        # a fully masked tile pools to sums 0 and maxima 0 (not -inf), and masked rows are exactly zero
        assert float(t["part"][1, 2].abs().max()) == 0.0
        assert float((t["layer0"] * (1 - torch.from_numpy(mask))[..., None]).abs().max()) == 0.0
    _hold(name, prec, _stages(name, prec, variant, sd, ids, mask, D, t))
    ref = mr.mamba_forward_fp64(variant, sd, ids, mask=mask, device="cuda").cpu()
    assert float((t["logits"].double() - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(SCALES))
def test_activation_scale_axis(built_lib, name, prec):
    """Exact fp32 is fp32 class at every scale.  The fp16x3 projections are held to what the FORMAT gives (the split model); the
    printed model / float32 ratio shows where the format leaves fp32 class."""
    variant, sd, ids, mask, D, t = _forward(SCALES[name], prec)
    _hold(name, prec, _stages(name, prec, variant, sd, ids, mask, D, t, split=True))
    if prec == "fp16x3":
        p32, p64 = S.layer_params(variant, sd, 0, torch.float32), S.layer_params(variant, sd, 0, torch.float64)
        h64, g64, q64 = t["front"].double(), t["g"].double(), t["ssq"].double()
        post = lambda y: S.out_proj_post(p64, h64, y.double(), q64)        # noqa: E731
        W, Wo = p32["in_proj.weight"], S.out_weight(p32)
        trios = (("in_proj", t["front"], (h64 @ W.double().T)[..., :D.dt0], em.x3_linear(t["front"], W)[..., :D.dt0],
                  (t["front"] @ W.T)[..., :D.dt0]),
                 ("out_proj", t["g"], post(g64 @ S.out_weight(p64).T), post(em.x3_linear(t["g"], Wo)), post(t["g"] @ Wo.T)))
        rows = []
        rms = lambda v: float(v.pow(2).mean().sqrt())                      # noqa: E731
        for stage, a, ref, model, f32 in trios:
            sm, sf = S.statistic(model, ref), S.statistic(f32, ref)
            rows.append(f"SPLIT {name:14s} {stage:9s} median |input| {float(a.abs().median()):.1e}  split model max {float(sm.max()):.2e} "
                        f"rms {rms(sm):.2e}  float32 product max {float(sf.max()):.2e} rms {rms(sf):.2e}  model / float32 (rms) "
                        f"{rms(sm) / max(rms(sf), 1e-300):8.1f}")
        _record(rows)


def test_conv_and_scan_are_one_code_in_both_precisions(built_lib):
    """Conv and scan are exact fp32 in both precisions: given equal inputs their outputs are bit-equal.  Equal inputs come from
    weights on a coarse grid (in_proj on multiples of 2^-8 below 1, the embedding on multiples of 2^-4 below 8): every product and
    every partial sum of in_proj is then exact in fp32 AND in the split format, so both precisions compute the same zx."""
    sd = mr.make_mamba_state_dict("mambasp", 52, n_layers=1, d_model=256, expand=2, d_state=64)
    sd["embedding.weight"] = (sd["embedding.weight"] * 16).round().clamp(-127, 127) / 16
    sd["mamba_layers.0.in_proj.weight"] = (sd["mamba_layers.0.in_proj.weight"] * 256).round().clamp(-255, 255) / 256
    got = {prec: _forward(lambda: ("mambasp", sd, _sp_ids(5300, 3, 129), None), prec)[-1] for prec in PRECS}
    a, b = got["fp32"], got["fp16x3"]
    assert torch.equal(a["zx"], b["zx"]), "precondition: in_proj is exact on this grid in both precisions"
    for k in ("xc", "g", "ssq"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["layer0"], b["layer0"])            # (out_proj is where the two differ)


@pytest.mark.parametrize("prec", PRECS)
def test_taps_are_deterministic(built_lib, prec):
    make = CASES["sp-e3-N32-L1031"]
    a, b = _forward(make, prec)[-1], _forward(make, prec)[-1]
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_tap_names_and_sizes(built_lib):
    from chimeralm_amd.mamba import MambaEngineError

    variant, sd, ids, mask = _sp_case(1, 16, 65)()
    net, D = _net(variant, sd, "fp32")
    B, L = ids.shape
    net(torch.from_numpy(ids).cuda())
    # the whole batch ran as one chunk of reads by the ABI's own arithmetic (the in_proj output of a chunk is bounded at 4 GiB)
    assert min(B, ((4 << 30) // (D.n_in_pad * 4)) // L) == B
    assert D.n_in == 548 and D.n_in_pad == 768
    for name, shape in (("zx", (B, L, 768)), ("xc", (B, L, 288)), ("g", (B, L, 256)), ("ssq", (B, L, 4)), ("part", (B, 2, 2, 256))):
        assert np.isfinite(net.debug_fetch(name, shape)).all()
        with pytest.raises(MambaEngineError, match="more bytes requested"):
            net.debug_fetch(name, (int(np.prod(shape)) + 1,))
    with pytest.raises(MambaEngineError, match="unknown name"):
        net.debug_fetch("y", (1,))
    net.close()
