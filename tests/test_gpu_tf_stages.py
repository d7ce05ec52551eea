"""GPU (MI355X): every kernel a SequenceCNNTransformer forward launches against float64, stage by stage and POSITION BY POSITION.

tests/test_gpu_transformer.py sees these kernels through two logits, `pooled` and one max-abs figure over the twelfth layer (2e-4 on
a stream of magnitude 1: a thousand fp32 roundings, and a maximum over the whole tensor).  Here a case is one seeded one- or two-layer
net (the production net runs exactly these kernel instances in every layer), one batch, one precision, a handful of STOPPED forwards
(`clm_tf_debug_stop_after`) and a full one; after each the workspace is fetched (`clm_tf_debug_fetch`) and every stage is compared,
every position of it, with tests/tf_stage_reference.py evaluated in float64 on the engine's OWN fetched input of that stage:
    x0 (exact path: bit-equal to embedding.weight[ids]) -> x1 -> x2 -> x3 (the stem levels) -> pe_ln -> in{i}.q / .k / .v (in_proj,
    each third over its own row maximum) -> att{i} -> layer{i} (out_proj + LN1 + feed-forward + LN2) -> scores, pooled, logits.
The attention is compared in its place in the chain, so a wrong hand-over of qkv or att shows: in the exact modes against the float32
yardstick, in the 16-bit modes against tests/attention_reference.py's model and bound (ratio <= 1); no new claim about it is made.

KERNEL -> CASES.  Exact path (fp32 and fp16x3 each): tf32::embed_kernel x0, every case; conv32_kernel<AR>, three launches x1 / x2 / x3, every
case; tf32::ln_kernel with pe pe_ln, every case; enc32_kernel<true, AR> (in_proj only) in0.*, every case; enc32_kernel<false, AR> without a
next in_proj layer0 of the one-layer cases and layer1 of 2layers, with it layer0 + in1.* of 2layers.  16-bit path (fp16, bf16, fp16c
each): conv3_relu_pool_kernel<PREC, true> x1, <PREC, false> x2 / x3; pe_ln_kernel pe_ln and hx; linear16_kernel in0.*; enc_ffn16_kernel in
its whole-layer form layer0 (without a next in_proj) and, in 2layers, layer0 + in1.* (with it) and layer1; fp16c's two-plane att and
its 1 / 64 in every fp16c case.  Both paths: pool_head_kernel scores / pooled / logits, every case.

STATISTIC.  Per position: max_c |got - ref| / max_c |ref|, the row's own maximum as denominator (scores: per read over max |score|; a
zero denominator demands an exact result, and the ReLU zeros of the dead-channel regime are asserted to be exact zeros).  Per read, the
max and the rms over positions.  No position is left out.  BOUND: engine <= max(K x the same statistic of the yardstick, 32 x 2^-24).
Yardsticks: fp32, and fp16x3 at unit scale -- the same stage in float32 on the CPU on the same input (K32); the fp16x3 projections and
attention of the activation-scale sweep -- the split model of the format (error_model.x3_linear, tf_stage_reference.attention_x3;
K_SPLIT); fp16, bf16, fp16c -- the 16-bit model of the stage (K16); the fp32 kernels of the 16-bit path (pe_ln, the head) -- float32.

BIT-EXACT RELATIONS, asserted as such: a stopped forward's buffers equal those of a forward stopped later, until a later launch
rewrites them; x0 equals the embedding rows; hx equals hidden rounded once to the element type; the head's scores, pooled and logits
are those stages computed from the fetched hidden (within the bound).

SHAPES.  d 256, B = 3: read 0 left-padded to its last token, read 1 without pads, read 2 with 3 pads and one N.  L = 8 (also B = 1: one
position per read, M = 3 / 1, one key), 15 (a trailing position dropped at every level), 129, 130 (the 16-bit stem's second tile holds one
input and no output / two and one), 511, 512 (M = 189, 192: layer tiles straddle reads; whole tiles), 527 (every level odd, M = 195:
ragged last tile in both paths, pe wraps inside a tile), 1039 (129 positions: 128-query tile plus one), 2055 (M = 768, full tiles); all
five precisions at 8, 15, 130, 527, 1039, fp32 and fp16x3 at the rest; two layers at 527.  REGIMES at 3 x 527
(tf_stage_reference.regime_state_dict; tests/test_tf_stage_host.py holds the float32 yardstick below 1e-3 in each): dead channels,
peaked and flat attention, sublayer scale (x 2^-6 and x 8), peaked pooling (fp32, fp16x3; the first three -- dead, attention, sublayer
scale: five settings -- also fp16c, fp16); the fp16x3
activation-scale axis, v rows of in_proj x 2^0, 2^-4, 2^-8, 2^-12.

K, from the first run (no bound set before it; profiles/tf_stage_parity.txt).  Three kinds of figure exceeded 8 x the float32 yardstick:
  (1) the layer stage of enc32_kernel: 9.66 (fp32) and 8.06 (fp16x3) with the sublayers x 2^-6, 3 - 5 everywhere else.  A DEFECT: the
      out_proj accumulators were preset to h + b_o and x1 stayed in the fc2 accumulators, so every MFMA step rounded at the residual's
      magnitude.  Fixed in this change (both sums start from zero, the residual waits in registers of its own and is added once; no
      scratch, the same occupancy): 1.13 / 1.31 at 2^-6, <= 3.0 everywhere; rms over positions / yardstick rms per regime, before -> after,
      fp32 | fp16x3: unit 3.78 -> 1.69 | 3.17 -> 1.36, dead 3.83 -> 1.81 | 3.27 -> 1.53, peaked 3.34 -> 1.65 | 2.75 -> 1.34, flat 3.38 -> 1.62 |
      3.05 -> 1.50, 2^-6 8.05 -> 1.01 | 6.78 -> 0.99, x 8 1.97 -> 2.03 | 1.70 -> 1.72, pool16 3.53 -> 1.79 | 2.96 -> 1.41.
  (2) fp16x3's attention with v x 2^-12: 61 x float32.  The FORMAT: attention_x3_kernel splits v unscaled, and |v| ~ 2e-4 has no lo half
      left in fp16 (2.6e-5 of the row maximum).  Held to the split model in the sweep since (engine / model 1.00); against float32 (rms)
      0.8 at median |att| 8e-1 and 5e-2, 3.6 at 3e-3, 57 at 2e-4.  The LAYER stage stays in fp32 class at every scale (split model /
      float32 0.6 - 0.7): out_proj's product of a small att lands on an order-1 residual.
  (3) figures far below the floor over one or two numbers whose float32 yardstick is tiny, or exactly zero, by chance: the logits (two per
      read; engine <= 1.0e-6, the 256-term sequential fmaf chain of pool_head_kernel; ratio up to 24), the scores of one-position reads
      (ratio up to 10 at 7e-8) and the attention of one-position reads (the float32 softmax over one key returns v exactly, the kernels
      are one rounding off: 5.5e-8 / 1.1e-7, ratio inf).  The floor is there for these.
After the fix the worst ratio among figures above the floor is 3.46 against float32, and 6.76 among all figures of more than two numbers
(the stem at 2,055 tokens: 768 sequential MFMA steps against a blocked CPU sum) -> K32 = 16, the smallest power of two >= 2 x 6.76 and the
cap; 1.25 against the 16-bit models (fp16c's layer at L = 15: its lo product reads the activation truncated to e5m2, which the model
leaves out; <= 1.03 otherwise) -> K16 = 4; 5.00 against the split model (in_proj at unit scale: the model accumulates in fp64) ->
K_SPLIT = 8, the cap.  (The sublayer-scale regime in fp16c / fp16: layer stage 1.05, 1.14 / 1.01, 1.00.)

WHAT HOLDS THE FIX of (1).  The unfixed kernel's damage is an rms of about 1e-6 of the row maximum: below the floor, so the bound above
passes it.  `_hold_layer_rms` therefore holds the layer stage of fp32 and fp16x3 in the regimes with small sublayers (sub2^-6, flat), per
read, to engine rms <= K_LAYER_RMS x the float32 yardstick's rms WITHOUT the floor; K_LAYER_RMS = 4 by the same rule (fixed kernel:
0.96 - 1.06 at 2^-6, 1.39 - 1.65 at flat).  Run once against this tree linked with the kernel as it was: 7.88 - 8.27 (fp32), 6.58 - 7.05
(fp16x3) at 2^-6, and exactly test_regimes[fp32-sub2^-6] and [fp16x3-sub2^-6] fail; at flat attention the old kernel measures 2.94 - 3.48,
inside 4, so there the assertion guards and the 2^-6 regime decides.

MEASURED on the MI355X, this tree: the worst engine / yardstick ratio over cases, reads and both statistics (all figures | those above
the floor), with that case's largest per-position errors.  The whole file: 75 tests in 6.1 s.
  float32 yardstick                                               16-bit stage model
    precision stage   all    above  engine max  yardstick           precision stage   all    above  engine max  yardstick
    fp32      x       6.76   -      1.60e-06    2.87e-07            fp16      x       1.01   1.01   5.58e-04    5.58e-04
    fp32      pe_ln   1.25   -      2.00e-07    2.00e-07            fp16      in.*    1.00   1.00   5.25e-04    5.25e-04
    fp32      in.*    5.50   -      9.15e-07    2.16e-07            fp16      layer   1.01   1.01   3.67e-04    3.67e-04
    fp32      att     inf    1.33   1.12e-05    1.11e-05            bf16      x       1.00   1.00   3.95e-03    3.95e-03
    fp32      layer   3.00   -      8.77e-07    3.34e-07            bf16      in.*    1.00   1.00   3.87e-03    3.87e-03
    fp32      scores  7.48   -      7.37e-08    2.11e-07            bf16      layer   1.00   1.00   3.13e-03    3.13e-03
    fp32      pooled  1.90   -      1.69e-07    1.25e-07            fp16c     x       1.03   1.03   4.24e-04    4.24e-04
    fp32      logits  15.79  -      4.81e-07    1.22e-07            fp16c     in.*    1.02   1.02   5.52e-04    5.52e-04
    fp16x3    x       6.53   -      1.87e-06    2.86e-07            fp16c     layer   1.25   1.25   2.12e-04    2.00e-04
    fp16x3    pe_ln   1.14   -      2.55e-07    2.23e-07          split model (fp16x3, activation-scale sweep)
    fp16x3    in.*    2.35   -      3.29e-07    1.40e-07            fp16x3    in.*    5.00   -      7.24e-07    1.52e-07
    fp16x3    att     inf    1.65   1.09e-05    1.45e-05            fp16x3    att     3.99   1.00   2.63e-05    2.63e-05
    fp16x3    layer   2.72   -      1.16e-06    5.39e-07            fp16x3    layer   4.00   -      9.47e-07    2.66e-07
    fp16x3    scores  0.99   -      1.54e-07    2.12e-07          fp32 kernels of the 16-bit path (float32 yardstick)
    fp16x3    pooled  2.01   -      8.36e-07    7.74e-07            pe_ln 1.30, pooled 1.62, scores 9.97 and logits 23.70 (3.46 above
    fp16x3    logits  18.86  -      8.42e-07    4.01e-07            the floor), all at engine <= 1.0e-6
("-": no figure of that stage reached the floor of 1.9e-6.)

SANITY of these tests, done once by hand on three wrong-on-purpose builds (never committed), the file's then 70 tests against each:
  a stem halo row taken from the neighbouring read instead of zero (both paths): 64 tests fail, each in x1, x2 and x3 and in no other
    stage; the B = 1 cases (no neighbour) and the fetch-name test pass;
  pe indexed by the flattened row (modulo 2 L3, to stay inside the table) instead of row % L3 (both paths): the same 64 fail, in pe_ln alone;
  the ragged-tile count of the layer kernels one short (both paths): 65 fail, in layer0 / layer1 and, on the exact path, whose in_proj
    form shares the count, in0.* / in1.*; the whole-tile cases (3 x 512, 3 x 2,055; fp32, fp16x3) pass.
Each build fails exactly the stage it breaks and passes exactly the cases its defect cannot reach.  (Whether the logit tests of
tests/test_gpu_transformer.py see these three was not measured; tests/test_tf_stage_host.py shows what its max-abs gate misses.)
"""
from __future__ import annotations

import os
import time

import numpy as np
import pytest
import torch

import attention_reference as A
import error_model as em
import tf_stage_reference as S
from tf_stage_reference import REGIMES, REGIMES_16, V_SCALES

pytestmark = pytest.mark.gpu

K32 = 16                    # x the float32 yardstick (fp32 everywhere; fp16x3 at unit scale; the fp32 kernels of the 16-bit path)
K16 = 4                     # x the 16-bit stage model (fp16, bf16, fp16c)
K_SPLIT = 8                 # x the split-model yardstick (fp16x3 projections of the activation-scale sweep)
K_LAYER_RMS = 4             # x the float32 yardstick's rms, WITHOUT the floor: the exact layer kernel where its sublayers are small
SMALL_SUBLAYER = ("sub2^-6", "flat")
EXACT_PRECS = ("fp32", "fp16x3")
PRECS16 = ("fp16", "bf16", "fp16c")
MODE16 = {"fp16": "fp16", "bf16": "bf16", "fp16c": "hilo"}      # attention_reference's names
TILE = {True: 64, False: 128}                                     # rows per tile of the layer kernels: exact path, 16-bit path


# ------------------------------------------------------------------------------------------------------------- one case
def _net(sd, prec):
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(vocab_size=12, max_len=sd["pos_encoder.pe"].shape[1], num_encoder_layers=S.n_layers_of(sd),
                                 precision=prec, selfcheck=False)
    net.load_state_dict(sd, strict=True)
    return net


def _fetch(net, prec, name, shape):
    """A buffer as a CPU tensor in its storage type (fp32, fp16 or bf16)."""
    if prec in EXACT_PRECS or name in ("hidden", "scores", "pooled"):
        return torch.from_numpy(net.debug_fetch(name, shape))
    raw = torch.from_numpy(net.debug_fetch(name, shape, np.int16))
    return raw.view(torch.bfloat16 if prec == "bf16" else torch.float16)


def _forwards(sd, ids, prec):
    """The stopped forwards and the full one of a case: taps[(stop, name)] and the logits."""
    exact = prec in EXACT_PRECS
    nl = S.n_layers_of(sd)
    B, L = ids.shape
    L1, L2, L3 = L // 2, L // 4, L // 8
    shapes = {"x0": (B, L, 256), "x1": (B, L1, 256), "x2": (B, L2, 256), "x3": (B, L3, 256), "hidden": (B, L3, 256), "hx": (B, L3, 256),
              "qkv": (B, L3, 768), "att": (2, B, L3, 256) if prec == "fp16c" else (B, L3, 256), "scores": (B, L3), "pooled": (B, 256)}
    acts = ("x2", "x3", "hidden", "qkv", "att") if exact else ("x1", "x2", "x3", "hx", "hidden", "qkv", "att")
    plan = [("conv1", ("x0", "x1")), ("conv2", ("x1", "x2"))] if exact else []
    plan.append((("attention", 0), acts))
    for i in range(1, nl):
        plan.append((("layer", i - 1), tuple(n for n in acts if n != "att")))
        plan.append((("attention", i), acts))
    plan.append((None, acts + ("scores", "pooled")))
    net = _net(sd, prec)
    dev = torch.from_numpy(ids).cuda()
    taps, logits = {}, None
    for stop, names in plan:
        net.debug_stop_after(stop)
        out = net(dev)
        for n in names:
            taps[(stop, n)] = _fetch(net, prec, n, shapes[n])
        if stop is None:
            logits = out.cpu()
    if prec != "fp32":
        assert net.precision_report["fallback"] is False
    net.close()
    return taps, logits


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_TF_STAGE_PARITY"):
        with open(os.environ["CLM_TF_STAGE_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _bit_exact(taps, prec, nl):
    """A stopped forward's buffers are those of a forward stopped later, until a later launch rewrites them."""
    first = {}
    rewritten = {("layer", i): ("hidden", "hx", "qkv") for i in range(nl)}
    rewritten.update({("attention", i): ("att",) for i in range(1, nl)})
    rewritten[None] = ("hidden", "hx")                          # the last layer's kernel
    for (stop, name), t in taps.items():
        if name in rewritten.get(stop, ()) or name not in first:
            first[name] = (stop, t)
            continue
        assert torch.equal(first[name][1], t), f"{name}: after stop {stop} not what it was after stop {first[name][0]}"
    if prec in PRECS16:
        for (stop, name), t in taps.items():
            if name == "hx":
                assert torch.equal(taps[(stop, "hidden")].to(t.dtype), t), f"hx after stop {stop}: not `hidden` rounded once"


def _stages(prec, sd, ids, taps, logits, split=False):
    """(stage, engine statistic, yardstick statistic, K, tile) of every stage of the case, each on the ENGINE's fetched input."""
    exact = prec in EXACT_PRECS
    nl = S.n_layers_of(sd)
    last = nl - 1
    w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
    idt = torch.from_numpy(ids)
    up = lambda x: x.double()                                   # noqa: E731
    fmt = S.EXACT if exact else S.FORMATS[prec]
    use_split = split and prec == "fp16x3"
    lin = (lambda a, W: em.x3_linear(a, W).float()) if use_split else None
    kp = K_SPLIT if use_split else K32 if exact else K16
    tile = TILE[exact]
    out = []

    def add(stage, got, ref, yard, k, tl=None, den=None):
        out.append((stage, S.statistic(up(got), ref, den), S.statistic(up(yard), ref, den), k, tl))

    def stem(c, x_in, got):
        """Level c: exact modes on the fetched fp32 rows with the float32 yardstick, 16-bit modes against their model."""
        if exact:
            add(f"x{c + 1}", got, S.stem_level(w64, c, up(x_in)), S.stem_level(w32, c, x_in), K32, 32)
        else:
            add(f"x{c + 1}", got, S.stem_level(w64, c, up(x_in)), S.stem_level(w64, c, up(x_in), fmt), K16, 64)

    # ---- stem
    emb = S.embed(w32, idt)
    a0 = ("attention", 0)
    if exact:
        assert torch.equal(taps[("conv1", "x0")], emb), "x0: not the embedding's rows"
        stem(0, taps[("conv1", "x0")], taps[("conv1", "x1")])
        stem(1, taps[("conv1", "x1")], taps[("conv2", "x2")])
    else:
        stem(0, emb, taps[(a0, "x1")])
        stem(1, taps[(a0, "x1")], taps[(a0, "x2")])
    stem(2, taps[(a0, "x2")] if not exact else taps[("conv2", "x2")], taps[(a0, "x3")])
    # ---- + pe, LayerNorm (an fp32 kernel in both paths)
    x3 = taps[(a0, "x3")]
    add("pe_ln", taps[(a0, "hidden")], S.pe_ln(w64, up(x3)), S.pe_ln(w32, x3.float()), K32, 4)
    # ---- the layers
    h_stop = a0
    for i in range(nl):
        ai = ("attention", i)
        h_in = taps[(h_stop, "hidden")]                         # layer i's input: what layer i - 1's kernel (or pe_ln) left
        qkv = taps[(h_stop, "qkv")]                             # ... and the in_proj handed over with it
        q64 = S.in_proj(w64, i, up(h_in))
        q_y = S.in_proj(w32, i, h_in, lin=lin) if exact else S.in_proj(w64, i, up(h_in), fmt)
        for g, name in enumerate("qkv"):                        # q, k and v rows each against their own maximum
            sl = slice(256 * g, 256 * g + 256)
            add(f"in{i}.{name}", qkv[..., sl], q64[..., sl], q_y[..., sl], kp, tile)
        att = taps[(ai, "att")]
        if exact:                                               # (the sweep: fp16x3's attention against the format's model as well)
            add(f"att{i}", att, S.attention(up(qkv)), S.attention_x3(qkv) if use_split else S.attention(qkv), kp if use_split else K32, 128)
            att_in, att_y = up(att), att
        else:                                                   # the attention kernel's own model and bound, in its place in the chain
            ref, tol = A.reference_and_bound(qkv, MODE16[prec])
            r = A.worst_ratio(A.to_float64(att, MODE16[prec]), ref, tol)
            assert r <= 1.0, f"att{i}: {r:.3g} x the bound of tests/attention_reference.py"
            att_in = A.to_float64(att, MODE16[prec])
            att_y = (up(att[0]), up(att[1])) if prec == "fp16c" else up(att)
        o_stop = ("layer", i) if i < last else None
        ref = S.layer_tail(w64, i, up(h_in), att_in)
        yard = S.layer_tail(w32, i, h_in, att_y, lin=lin) if exact else S.layer_tail(w64, i, up(h_in), att_y, fmt)
        add(f"layer{i}", taps[(o_stop, "hidden")], ref, yard, kp, tile)
        h_stop = o_stop
    # ---- the head runs on what the layers left (an fp32 kernel in both paths)
    h = taps[(None, "hidden")]
    sc64 = S.pool_scores(w64, up(h))
    add("scores", taps[(None, "scores")], sc64, S.pool_scores(w32, h), K32, den=sc64.abs().amax(1))
    add("pooled", taps[(None, "pooled")][:, None], S.pooled(w64, up(h))[:, None], S.pooled(w32, h)[:, None], K32)
    pl = taps[(None, "pooled")]
    add("logits", logits[:, None], S.logits(w64, up(pl))[:, None], S.logits(w32, pl)[:, None], K32)
    return out


def _hold(tag, prec, stages):
    rows, bad, summary = [], [], []
    for stage, e, y, k, tile in stages:
        worst, above = S.check(f"{tag} {prec}", stage, e, y, k, rows, bad, tile)
        summary.append(f"STAGE {tag:24s} {prec:6s} {stage:8s} engine max {float(e.max()):.2e} rms {float(e.pow(2).mean().sqrt()):.2e}  "
                       f"yardstick max {float(y.max()):.2e} rms {float(y.pow(2).mean().sqrt()):.2e}  K {k}  worst ratio {worst:6.2f}  above the floor {above:6.2f}")
    print("\n".join(rows))
    _record(summary)
    assert not bad, "\n".join(bad)


def _case(tag, prec, sd, ids, split=False):
    t0 = time.time()
    taps, logits = _forwards(sd, ids, prec)
    for t in list(taps.values()) + [logits]:
        assert bool(torch.isfinite(t.float()).all())
    _bit_exact(taps, prec, S.n_layers_of(sd))
    stages = _stages(prec, sd, ids, taps, logits, split)
    _hold(tag, prec, stages)
    print(f"TIME {tag} {prec}: {time.time() - t0:.2f} s")
    return taps


def _hold_layer_rms(tag, prec, sd, taps):
    """What holds enc32_kernel's sublayer sums to start from zero.  Summed onto the residual, every MFMA step rounds at the residual's
    magnitude; the damage (3 - 8 x the float32 yardstick) is an rms of about 1e-6 of the row maximum, BELOW the floor of 1.9e-6 that the
    general bound falls back to, so that bound passes it.  Here, where the sublayers are small against the stream (out_proj and linear2
    x 2^-6; att = the mean of v), the layer stage's rms over the positions of each read is held to K_LAYER_RMS x the float32 yardstick's
    rms with no floor.  K_LAYER_RMS by the rule of the module docstring: the fixed kernel's worst such ratio is 1.62, 2 x 1.62 -> 4
    (the kernel before the fix: 8.05 / 6.78 with the sublayers x 2^-6, 3.38 / 3.05 at flat attention)."""
    w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
    a0 = ("attention", 0)
    h, att = taps[(a0, "hidden")], taps[(a0, "att")]
    ref = S.layer_tail(w64, 0, h.double(), att.double())
    _, e_rms = S.read_stats(S.statistic(taps[(None, "hidden")].double(), ref))
    _, y_rms = S.read_stats(S.statistic(S.layer_tail(w32, 0, h, att), ref))
    rows = [f"LAYER-RMS {tag:18s} {prec:6s} read {b}: engine rms {e:.3e}  yardstick rms {y:.3e}  ratio {e / y:5.2f}  K {K_LAYER_RMS}"
            for b, (e, y) in enumerate(zip(e_rms, y_rms))]
    _record(rows)
    bad = [r for r, e, y in zip(rows, e_rms, y_rms) if not e <= K_LAYER_RMS * y]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------- the cases
SHAPES_ALL = [(3, 8), (1, 8), (3, 15), (3, 130), (3, 527), (3, 1039)]
SHAPES_EXACT = [(3, 129), (3, 511), (3, 512), (3, 2055)]
SHAPE_CASES = [(p, B, L) for p in EXACT_PRECS + PRECS16 for (B, L) in SHAPES_ALL] + [(p, B, L) for p in EXACT_PRECS for (B, L) in SHAPES_EXACT]


@pytest.mark.parametrize("prec,B,L", SHAPE_CASES)
def test_every_stage_every_position(built_lib, prec, B, L):
    _case(f"1layer-B{B}-L{L}", prec, S.make_net(64), S.stage_ids(6400 + L, B, L))


@pytest.mark.parametrize("prec", EXACT_PRECS + PRECS16)
def test_two_layers_hand_the_in_proj_over(built_lib, prec):
    """Layer 0's kernel in its with-next form: its LN2 tile feeds layer 1's in_proj, whose qkv layer 1's attention reads."""
    _case("2layers-B3-L527", prec, S.make_net(65, layers=2), S.stage_ids(6500, 3, 527))


@pytest.mark.parametrize("prec,regime", [(p, r) for p in EXACT_PRECS for r in REGIMES] + [(p, r) for p in ("fp16c", "fp16") for r in REGIMES_16])
def test_regimes(built_lib, prec, regime):
    sd = S.regime_state_dict(regime)
    ids = S.stage_ids(6000, 3, 527)
    taps = _case(f"regime-{regime}", prec, sd, ids)
    if prec in EXACT_PRECS and regime in SMALL_SUBLAYER:
        _hold_layer_rms(f"regime-{regime}", prec, sd, taps)
    if regime == "dead":                                        # the ReLU zeros of the stem are exact zeros
        for (stop, name), t in taps.items():
            if name in ("x1", "x2", "x3"):
                assert float(t[..., 1::2].float().abs().max()) == 0.0, (stop, name)


@pytest.mark.parametrize("prec", EXACT_PRECS)
@pytest.mark.parametrize("k", V_SCALES)
def test_activation_scale_axis(built_lib, k, prec):
    """The v rows of in_proj x 2^-k: a small att under an order-1 stream.  Exact fp32 is fp32 class at every scale; the fp16x3 projections
    are held to what the FORMAT gives (the split model), and the printed model / float32 ratio shows where it leaves fp32 class."""
    sd = S.regime_state_dict(f"v2^-{k}")
    ids = S.stage_ids(6000, 3, 527)
    taps = _case(f"scale-v2^-{k}", prec, sd, ids, split=True)
    if prec == "fp16x3":
        w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
        h, att = taps[(("attention", 0), "hidden")], taps[(("attention", 0), "att")]
        ref = S.layer_tail(w64, 0, h.double(), att.double())
        sm = S.statistic(S.layer_tail(w32, 0, h, att, lin=lambda a, W: em.x3_linear(a, W).float()), ref)
        sf = S.statistic(S.layer_tail(w32, 0, h, att), ref)
        rms = lambda v: float(v.pow(2).mean().sqrt())           # noqa: E731
        _record([f"SPLIT scale-v2^-{k:<2d} layer0  median |att| {float(att.abs().median()):.1e}  split model max {float(sm.max()):.2e} rms "
                 f"{rms(sm):.2e}  float32 max {float(sf.max()):.2e} rms {rms(sf):.2e}  model / float32 (rms) {rms(sm) / max(rms(sf), 1e-300):8.2f}"])


def test_the_separate_fp32_launches_refuse_the_stop_and_the_fused_names(built_lib, monkeypatch):
    """CLM_DEBUG=unfused_fp32 lays the exact path's workspace out differently: no stop, and of the fetch names only the shared ones."""
    from chimeralm_amd.transformer import TransformerEngineError

    monkeypatch.setenv("CLM_DEBUG", "unfused_fp32")             # read by clm_tf_create
    net = _net(S.make_net(64), "fp32")
    ids = torch.from_numpy(S.stage_ids(6401, 3, 130)).cuda()
    assert bool(torch.isfinite(net(ids)).all())
    assert np.isfinite(net.debug_fetch("hidden", (3, 16, 256))).all() and np.isfinite(net.debug_fetch("scores", (3, 16))).all()
    for name, shape in (("x0", (3, 130, 256)), ("x1", (3, 65, 256)), ("x2", (3, 32, 256)), ("x3", (3, 16, 256)), ("qkv", (3, 16, 768)),
                        ("att", (3, 16, 256))):
        with pytest.raises(TransformerEngineError, match="did not produce"):
            net.debug_fetch(name, shape)
    with pytest.raises(TransformerEngineError, match="fused launches only"):
        net.debug_stop_after("conv1")
    net.close()


def test_stops_and_fetch_names(built_lib):
    from chimeralm_amd.transformer import TransformerEngineError

    sd = S.make_net(64)
    ids = torch.from_numpy(S.stage_ids(6401, 3, 130)).cuda()
    for prec in ("fp32", "fp16"):
        net = _net(sd, prec)
        whole = net(ids).cpu()
        net.debug_fetch("scores", (3, 16))
        net.debug_stop_after("conv2")
        net(ids)
        for name, shape in (("scores", (3, 16)), ("pooled", (3, 256)), ("hidden", (3, 16, 256)), ("qkv", (3, 16, 768)), ("x3", (3, 16, 256))):
            with pytest.raises(TransformerEngineError, match="did not produce"):
                net.debug_fetch(name, shape)
        with pytest.raises(TransformerEngineError, match="did not produce"):
            net.debug_fetch("x0" if prec == "fp16" else "hx", (1,))
        np16 = np.float32 if prec == "fp32" else np.float16
        assert np.isfinite(net.debug_fetch("x2", (3, 32, 256), np16).astype(np.float32)).all()
        with pytest.raises(TransformerEngineError, match="more bytes requested"):
            net.debug_fetch("x2", (3 * 32 * 256 + 1,), np16)
        with pytest.raises(TransformerEngineError, match="unknown name"):
            net.debug_fetch("y", (1,))
        with pytest.raises(TransformerEngineError, match="no such stage"):
            net.debug_stop_after(("attention", 1))                 # a one-layer net
        net.debug_stop_after(None)
        assert torch.equal(net(ids).cpu(), whole)                   # the stop leaves nothing behind
        net.close()
