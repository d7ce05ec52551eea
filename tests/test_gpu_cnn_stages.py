"""GPU (MI355X): every kernel a DNAConvNet inference forward launches against float64, stage by stage and POSITION BY POSITION.

tests/test_gpu_cnn.py sees these kernels through two logits (an absolute 1e-4 on a mean over L/64 rows pushed through two dense layers)
and through block0, block1 and pooled at one shape, each to 1e-5 of the TENSOR's maximum; block 2, whose kernel instantiation
(cnn_gemm7_kernel<true, *>) stores only per-tile sums, it never sees on its own.  Here a case is one seeded net, one batch, one precision
and one forward; afterwards "block0", "block1", "partial" and "pooled" are fetched (clm_cnn_debug_fetch) and every stage is compared,
every position of it, with tests/cnn_stage_reference.py evaluated in float64 on the engine's OWN fetched input of that stage:
    ids -> block0 (cnn_block0_kernel) | fetched block0 -> block1 (cnn_gemm7_kernel<false, AR>) | fetched block1 -> block 2's rows ->
    tile_sums against "partial", one row per tile (cnn_gemm7_kernel<true, AR>) | fetched partial -> pooled | fetched pooled -> logits
    (both cnn_head_kernel).
An error made upstream does not count against a stage, and a wrong hand-over between two kernels shows in the stage that reads it.

STATISTIC (tests/tf_stage_reference.py's).  Per position: max_c |got - ref| / max_c |ref|, the row's own maximum as denominator.  Per
read, the max and the rms over positions.  No position is left out.  BOUND, fp32 and fp16x3 alike:
engine <= max(K32 x the same statistic of the float32 yardstick -- the same stage in float32 on the CPU on the same input --, 32 x 2^-24).
tests/test_cnn_stage_host.py holds that yardstick below the old 1e-5 per position in every case here (at most 5.4e-7, `deep` 5.4e-6), so
the bound is 20 x tighter than the old one per position wherever it is not the floor, and shows what the old gates do and do not see of
five planted defects.  Every fp16x3 case asserts that the fp16x3 kernels ran (precision_report["fallback"] is False).

BIT-EXACT RELATIONS, asserted as such: two forwards give identical buffers (all four, and the logits); every buffer of read b in the
batch of 3 is that of the read run alone.  `pooled` against the in-order float32 sum of the fetched partials / L64 is held to the bound;
it WAS bit-equal in all 38 cases of the run below (printed, not asserted).

SHAPES (cnn_stage_reference.SHAPES, GEOMETRY: what each reaches is computed from L in tests/test_cnn_stage_host.py).  B = 3: read 0
[PAD] up to its last token (constant windows: exact ties in every max-pool), read 1 without pads, read 2 with 3 pads and one N.
L = 64 (also B = 1), 67, 127, 259, 263, 271, 272, 515, 519, 1039, 1075, 1091, 2099.  REGIMES at 3 x 1075: every BatchNorm weight negative;
BatchNorm bias -1.5 (GELU's non-monotonic range, row maxima of 0.16 - 0.45); block 0's BatchNorm x 2^-4, 2^-8, 2^-12 (block 1's input
small: its fp16x3 lo halfs are fp16 subnormals).

K32, from the first run (no bound set before it; profiles/cnn_stage_parity.txt).  The worst engine / yardstick ratio among figures of more
than two numbers is 8.42 (fp32, block1, 3 x 127, read 1: 2.19e-6 at one of 7 positions against a yardstick maximum of 2.60e-7) -> the
smallest power of two >= 2 x 8.42 is 32, CAPPED at 16: K32 = 16.  No stage exceeds the cap, and no kernel was changed.
  * Blocks 1 and 2 in fp32 sit at 3 - 6 x the yardstick (rms over positions: 9e-7 against 2.3e-7), in fp16x3 at 2 - 4 x (6e-7).  This is
    the ORDER OF THE SUM, not a defect: the accumulators start from zero (bias, BatchNorm and GELU follow on the finished sum), and
    K = 7 x 256 runs as one chain of 896 v_mfma_f32_32x32x2_f32 steps per output against the CPU's blocked sum.  The same chain
    emulated on the CPU (acc = fl32(acc + a b), tap-major, on block 1 of the 3 x 127 and 3 x 1039 cases) measures rms 2.9 - 5.8 x and
    max 2.6 - 7.3 x the yardstick with one rounding per product, 2.8 - 3.6 x and 2.2 - 4.7 x with one per two; the engine on the same
    two cases: rms 2.1 - 6.7 x, max 2.7 - 8.4 x.  fp16x3 takes 16 products per step (112 steps x 3) and sits lower.  With block 0's
    output scaled down (act2^-k) the convolution is small against the BatchNorm shift and block 1 is AT the yardstick (0.8 - 1.2 x)
    in both precisions.
  * Block 0 never exceeds the yardstick (its table is computed in float64); pooled is the yardstick, bit for bit.
  * The logits (two numbers per read, the floor's business): up to 9.83; 4.46 above the floor, on reads whose logits are small.
  * The `deep` regime: engine 8.9e-6 / 4.7e-6 (fp32 / fp16x3) at the worst position against a yardstick of 4.7e-6: ratio <= 2.0.
WHAT THE MATRIX UNIT DOES WITH SUBNORMAL HALFS (printed by test_regimes as FORMAT rows; fp16x3, block 0 x 2^-4 .. 2^-12, median |input| of
block 1 down to 8.9e-5): it KEEPS them.  engine / flush model (error_model.x3_linear(flush=True), rms) = 0.002 - 0.015, i.e. the engine is
70 - 500 x more accurate than a unit that flushed them would be; engine / split model 2.1 - 2.7 (block 1) and 4.2 - 8.0 (partial) -- the
model accumulates in float64, the engine's remainder is the fp32 chain above.  Against float32 the fp16x3 stages stay at 0.9 - 2.3 x at
every scale, so the float32 yardstick is the right bound for this format on this net and no stage is held to the split model.

MEASURED on the MI355X, this tree: the worst engine / yardstick ratio over cases, reads and both statistics (all figures | those above
the floor of 1.9e-6), with the largest per-position error of the engine and of the yardstick over all cases.  39 tests in 6 - 7 s.
    precision stage    all    above  engine max  yardstick max
    fp32      block0   1.00   -      3.66e-07    9.09e-07
    fp32      block1   8.42   8.42   8.89e-06    4.67e-06
    fp32      partial  7.94   -      1.31e-06    3.69e-06
    fp32      pooled   1.00   -      5.72e-08    5.72e-08
    fp32      logits   9.83   2.87   9.20e-06    7.05e-06
    fp16x3    block0   1.00   -      3.66e-07    9.09e-07
    fp16x3    block1   6.02   5.02   4.70e-06    4.67e-06
    fp16x3    partial  6.53   -      9.53e-07    2.86e-06
    fp16x3    pooled   1.00   -      5.66e-08    5.66e-08
    fp16x3    logits   8.09   4.46   6.82e-06    1.56e-05
("-": no figure of that stage reached the floor.)
"""
from __future__ import annotations

import os
import time

import numpy as np
import pytest
import torch

import cnn_reference as cr
import cnn_stage_reference as S
import error_model as em
from cnn_stage_reference import REGIMES, SCALE_REGIMES, SHAPES

pytestmark = pytest.mark.gpu

K32 = 16                    # x the float32 yardstick, fp32 and fp16x3 alike (the cap; the module docstring has the measurement)
PRECS = ("fp32", "fp16x3")
FETCH = ("block0", "block1", "partial", "pooled")


# ------------------------------------------------------------------------------------------------------------- one case
def _net(sd, prec):
    from chimeralm_amd.cnn import DNAConvNet

    net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                     hidden_dim=512, number_of_classes=2, dropout=0.1, precision=prec)
    net.load_state_dict(sd, strict=True)
    return net


def _shapes(B, L):
    g = S.geometry(L)
    return {"block0": (B, g["L4"], 256), "block1": (B, g["L16"], 256), "partial": (B, g["tiles2"], 256), "pooled": (B, 256)}


def _forward(net, ids):
    """One forward: every fetched buffer and the logits, as CPU tensors."""
    logits = net(torch.from_numpy(ids).cuda()).cpu()
    taps = {n: torch.from_numpy(net.debug_fetch(n, shp)) for n, shp in _shapes(*ids.shape).items()}
    taps["logits"] = logits
    return taps


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_CNN_STAGE_PARITY"):
        with open(os.environ["CLM_CNN_STAGE_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _stages(sd, ids, taps):
    """(stage, engine statistic, yardstick statistic) of every stage of the case, each on the ENGINE's fetched input."""
    w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
    idt = torch.from_numpy(ids)
    L64 = ids.shape[1] // 64
    b0, b1, part, pooled = (taps[n] for n in FETCH)
    out = []

    def add(stage, got, ref, yard):
        assert got.shape == ref.shape == yard.shape, (stage, got.shape, ref.shape, yard.shape)
        out.append((stage, S.statistic(got.double(), ref), S.statistic(yard.double(), ref)))

    add("block0", b0, S.block0(w64, idt), S.block0(w32, idt))
    add("block1", b1, S.block(w64, 1, b0.double()), S.block(w32, 1, b0))
    add("partial", part, S.tile_sums(S.block(w64, 2, b1.double())), S.tile_sums(S.block(w32, 2, b1)))
    in_order = S.pooled_from(part, L64)                        # float32, the head kernel's order
    add("pooled", pooled[:, None], S.pooled_from(part.double(), L64)[:, None], in_order[:, None])
    add("logits", taps["logits"][:, None], S.head(w64, pooled.double())[:, None], S.head(w32, pooled)[:, None])
    return out, bool(torch.equal(pooled, in_order))


def _hold(tag, prec, stages):
    rows, bad, summary = [], [], []
    for stage, e, y in stages:
        worst, above = S.check(f"{tag} {prec}", stage, e, y, K32, rows, bad)
        summary.append(f"STAGE {tag:16s} {prec:6s} {stage:8s} engine max {float(e.max()):.2e} rms {float(e.pow(2).mean().sqrt()):.2e}  "
                       f"yardstick max {float(y.max()):.2e} rms {float(y.pow(2).mean().sqrt()):.2e}  K {K32}  worst ratio {worst:6.2f}  "
                       f"above the floor {above:6.2f}")
    print("\n".join(rows))
    _record(summary)
    assert not bad, "\n".join(bad)


def _case(tag, prec, sd, ids):
    t0 = time.time()
    B = ids.shape[0]
    net = _net(sd, prec)
    taps = _forward(net, ids)
    if prec == "fp16x3":
        assert net.precision_report["fallback"] is False
    for n, t in taps.items():
        assert bool(torch.isfinite(t).all()), n
    # bit-exact relations: a second forward gives the same buffers; read b of the batch is that read run alone, in every buffer
    again = _forward(net, ids)
    for n, t in taps.items():
        assert torch.equal(again[n], t), f"{n}: two forwards differ"
    if B > 1:
        for b in range(B):
            alone = _forward(net, ids[b:b + 1])
            for n, t in taps.items():
                assert torch.equal(alone[n][0], t[b]), f"{n}: read {b} of the batch is not that read run alone"
    net.close()
    stages, bit_equal = _stages(sd, ids, taps)
    _record([f"POOLED {tag:16s} {prec:6s} bit-equal to the in-order float32 sum of the fetched partials / L64: {bit_equal}"])
    _hold(tag, prec, stages)
    print(f"TIME {tag} {prec}: {time.time() - t0:.2f} s")
    return taps


# ------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_every_stage_every_position(built_lib, B, L, prec):
    _case(f"shape-B{B}-L{L}", prec, cr.make_cnn_state_dict(S.SEED_SHAPES), S.stage_ids(6400 + L, B, L))


def _format_models(tag, sd, taps):
    """fp16x3 on small activations: the engine's blocks 1 and 2 next to the split model of the format (error_model.x3_linear on the
    7 x 256 im2col rows) and to the same model with fp16-subnormal halfs read as zero -- what the matrix unit does with them."""
    w64 = S.weights(sd, torch.float64)
    rms = lambda v: float(v.pow(2).mean().sqrt())              # noqa: E731
    rows = []
    for i, k_in, k_out in ((1, "block0", "block1"), (2, "block1", "partial")):
        x = taps[k_in].double()
        post = S.tile_sums if i == 2 else (lambda r: r)
        ref = post(S.block(w64, i, x))
        e = S.statistic(taps[k_out].double(), ref)
        m = S.statistic(post(S.block(w64, i, x, lin=em.x3_linear)), ref)
        fl = S.statistic(post(S.block(w64, i, x, lin=lambda a, W: em.x3_linear(a, W, flush=True))), ref)
        rows.append(f"FORMAT {tag:16s} {k_out:8s} median |input| {float(x.abs().median()):.1e}  engine max {float(e.max()):.2e} rms {rms(e):.2e}  "
                    f"split model max {float(m.max()):.2e} rms {rms(m):.2e}  flush model max {float(fl.max()):.2e} rms {rms(fl):.2e}  "
                    f"engine / split (rms) {rms(e) / rms(m):7.2f}  engine / flush (rms) {rms(e) / rms(fl):7.4f}")
    _record(rows)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(built_lib, regime, prec):
    """allneg, deep and the activation-scale axis (unit scale is test_every_stage_every_position's 3 x 1075), under the SAME float32 bound."""
    sd = S.regime_state_dict(regime)
    taps = _case(f"regime-{regime}", prec, sd, S.stage_ids(6000, *S.REGIME_SHAPE))
    if prec == "fp16x3" and regime in SCALE_REGIMES:
        _format_models(f"regime-{regime}", sd, taps)


def test_fetch_names(built_lib):
    from chimeralm_amd.cnn import CnnEngineError

    net = _net(cr.make_cnn_state_dict(S.SEED_SHAPES), "fp32")
    net(torch.from_numpy(S.stage_ids(6400, 3, 1091)).cuda())
    assert np.isfinite(net.debug_fetch("partial", (3, 2, 256))).all()
    for name, n in (("partial", 3 * 2 * 256), ("block1", 3 * 68 * 256), ("pooled", 3 * 256)):
        with pytest.raises(CnnEngineError, match="more bytes requested"):
            net.debug_fetch(name, (n + 1,))
    with pytest.raises(CnnEngineError, match="unknown name"):
        net.debug_fetch("block2", (1,))
    net.close()
