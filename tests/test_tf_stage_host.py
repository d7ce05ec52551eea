"""Host (no GPU): tests/tf_stage_reference.py against the oracle, and the statistic of tests/test_gpu_tf_stages.py against planted errors.

The planted errors are the kinds the GPU test exists for -- confined to one position, to the first row of a read inside a flattened
tile, to the last valid row of a ragged tile, to the output next to a dropped trailing position -- each at about 100 x the float32
yardstick of its row.  The per-position statistic names every one of them; the global max-abs gate of tests/test_gpu_transformer.py
(TOL_HIDDEN = 2e-4 on a stream of magnitude 1) sees none.  That pair is the argument for the GPU test, kept as a test."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

import tf_stage_reference as S
from oracle import transformer_oracle as to

TOL_HIDDEN = 2e-4           # tests/test_gpu_transformer.py, fp32 and fp16x3
K = 16
B, L = 3, 527               # levels 263, 131, 65: M = 195 flattened rows, a ragged last tile in both paths


@pytest.fixture(scope="module")
def chain():
    sd = S.make_net(61)
    ids = S.stage_ids(6100, B, L)
    tr: dict = {}
    S.forward(sd, ids, torch.float64, trace=tr)
    w32 = S.weights(sd, torch.float32)
    y = S.layer_tail(w32, 0, tr["embedded"].float(), tr["att0"].float())
    return sd, ids, tr, y


def test_the_chained_stages_are_the_oracle():
    sd = S.make_net(62, layers=2)
    ids = S.stage_ids(6200, B, L)
    cfg = to.Config(num_encoder_layers=2, max_len=512)
    want_tr, got_tr = {}, {}
    want = to.forward(torch.from_numpy(ids), sd, cfg, dtype=torch.float64, trace=want_tr)
    got = S.forward(sd, ids, torch.float64, trace=got_tr)
    assert float((got - want).abs().max()) <= 1e-12
    assert set(want_tr) == {"cnn0", "cnn1", "cnn2", "embedded", "layer0", "layer1", "pool_weights", "pooled"}
    for k, v in want_tr.items():
        assert got_tr[k].shape == v.shape and float((got_tr[k] - v).abs().max()) <= 1e-12, k


def _plant(ref, yard_out, b, t, direction=None):
    """The yardstick's output with row (b, t) moved so that its statistic is 100 x the yardstick's maximum over read b."""
    y_stat = S.statistic(yard_out, ref)
    size = 100.0 * float(y_stat[b].max()) * float(ref[b, t].abs().max())
    got = yard_out.double().clone()
    if direction is None:
        direction = torch.zeros(ref.shape[-1], dtype=torch.float64)
        direction[37] = 1.0
    got[b, t] = ref[b, t] + size * direction / float(direction.abs().max())
    return got


PLANTS = {"one row of one position": (2, 17), "the first row of read 1": (1, 0), "the last valid row of a ragged tile": (2, L // 8 - 1)}


@pytest.mark.parametrize("kind", list(PLANTS))
def test_a_planted_row_error_is_named_and_the_global_gate_is_blind(chain, kind):
    sd, ids, tr, y = chain
    ref = tr["layer0"]
    b, t = PLANTS[kind]
    got = _plant(ref, y, b, t)
    rows, bad = [], []
    S.check("host", "layer", S.statistic(got, ref), S.statistic(y, ref), K, rows, bad, tile=64)
    assert bad and all(f"read {b} " in line for line in bad) and any(f"read {b} position {t} of" in line for line in bad), "\n".join(rows)
    assert float((got - ref).abs().max()) < TOL_HIDDEN              # what tests/test_gpu_transformer.py measures: inside its gate
    rows, bad = [], []
    S.check("host", "layer", S.statistic(y, ref), S.statistic(y, ref), K, rows, bad, tile=64)
    assert not bad                                                   # (and the unplanted rows pass)


def test_a_dropped_trailing_position_is_named_and_the_global_gate_is_blind(chain):
    """Level 0 of the stem on 527 rows keeps 263 outputs; the last one reads row 526, which the pooling drops, as its right neighbour.  A
    kernel that stops staging at the last kept input computes that output without it -- scaled here to 100 x the yardstick."""
    sd, ids, tr, _ = chain
    w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
    x0 = tr["x0"]
    ref = S.stem_level(w64, 0, x0)
    y = S.stem_level(w32, 0, x0.float())
    cut = x0.clone()
    cut[:, L - 1] = 0.0
    wrong = S.stem_level(w64, 0, cut)
    assert bool((wrong[:, :-1] == ref[:, :-1]).all()) and not bool((wrong[:, -1] == ref[:, -1]).all())
    for b in range(B):
        got = _plant(ref, y, b, L // 2 - 1, direction=(wrong - ref)[b, -1])
        rows, bad = [], []
        S.check("host", "x1", S.statistic(got, ref), S.statistic(y, ref), K, rows, bad, tile=32)
        assert any(f"read {b} position {L // 2 - 1} of" in line and "the last" in line for line in bad), "\n".join(rows)
        assert float((got - ref).abs().max()) < TOL_HIDDEN


def test_a_zero_denominator_demands_an_exact_result():
    ref = torch.zeros(1, 2, 4, dtype=torch.float64)
    got = ref.clone()
    assert float(S.statistic(got, ref).max()) == 0.0
    got[0, 1, 2] = 1e-30
    assert S.statistic(got, ref)[0].tolist() == [0.0, float("inf")]
    rows, bad = [], []
    S.check("host", "x", S.statistic(got, ref), S.statistic(ref, ref), K, rows, bad)
    assert bad


ALL_REGIMES = ("unit",) + S.REGIMES + tuple(f"v2^-{k}" for k in S.V_SCALES)


@pytest.mark.parametrize("regime", ALL_REGIMES)
def test_the_float32_yardstick_is_finite_and_small_in_every_regime(regime):
    """K x the yardstick means something only where the yardstick itself is small: every stage, every position, below 1e-3."""
    sd = S.make_net(60) if regime == "unit" else S.regime_state_dict(regime)
    ids = S.stage_ids(6000, B, L)
    tr: dict = {}
    S.forward(sd, ids, torch.float64, trace=tr)
    w32 = S.weights(sd, torch.float32)
    f = lambda k: tr[k].float()                                       # noqa: E731
    stages = {"x1": (S.stem_level(w32, 0, f("x0")), tr["x1"]), "x2": (S.stem_level(w32, 1, f("x1")), tr["x2"]),
              "x3": (S.stem_level(w32, 2, f("x2")), tr["x3"]), "pe_ln": (S.pe_ln(w32, f("x3")), tr["embedded"]),
              "in_proj": (S.in_proj(w32, 0, f("embedded")), tr["qkv0"]), "attention": (S.attention(f("qkv0")), tr["att0"]),
              "layer": (S.layer_tail(w32, 0, f("embedded"), f("att0")), tr["layer0"]),
              "pooled": (S.pooled(w32, f("layer0"))[:, None], tr["pooled"][:, None]),
              "logits": (S.logits(w32, f("pooled"))[:, None], S.logits(S.weights(sd, torch.float64), tr["pooled"])[:, None])}
    for name, (y, ref) in stages.items():
        st = S.statistic(y, ref)
        assert bool(torch.isfinite(st).all()) and float(st.max()) < 1e-3, (regime, name, float(st.max()))
    sc = S.statistic(S.pool_scores(w32, f("layer0")), tr["scores"], den=tr["scores"].abs().amax(1))
    assert bool(torch.isfinite(sc).all()) and float(sc.max()) < 1e-3
    if regime == "dead":
        for k in ("x1", "x2", "x3"):
            assert float(tr[k][..., 1::2].abs().max()) == 0.0 and float(stages[k][0][..., 1::2].abs().max()) == 0.0
    if regime == "flat":
        assert float((tr["att0"] - tr["att0"][:, :1]).abs().max()) < 1e-12     # the mean of v at every position


@pytest.mark.parametrize("prec", list(S.FORMATS))
def test_a_16bit_model_without_its_roundings_is_the_float64_stage(prec):
    sd = S.make_net(63)
    ids = S.stage_ids(6300, 2, 130)
    off = dataclasses.replace(S.FORMATS[prec], act=None, w=None)      # (fp16c keeps its two planes and its 1 / 64)
    a, b = {}, {}
    la, lb = S.forward(sd, ids, torch.float64, trace=a), S.forward(sd, ids, torch.float64, fmt=off, trace=b)
    assert torch.equal(la, lb)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    on: dict = {}
    S.forward(sd, ids, torch.float64, fmt=S.FORMATS[prec], trace=on)
    u = 2.0 ** -8 if prec == "bf16" else 2.0 ** -11
    for k in ("x1", "x3", "embedded", "qkv0", "layer0"):
        d = float(S.statistic(on[k], a[k]).max())
        assert 0.0 < d < 64 * u, (k, d)                              # ... and with them it is a 16-bit computation


def test_the_module_stage_codes_are_the_header_ones():
    """chimeralm_amd/transformer.py repeats the CLM_TF_STAGE_* codes of include/chimeralm_hip.h; this keeps the two from drifting."""
    import re
    from pathlib import Path

    from chimeralm_amd.transformer import SequenceCNNTransformer as T

    hdr = (Path(__file__).resolve().parent.parent / "include" / "chimeralm_hip.h").read_text()
    enum = {k.lower(): int(v) for k, v in re.findall(r"CLM_TF_STAGE_([A-Z0-9_]+) = (\d+)", hdr)}
    assert enum == T.TF_STOPS and len(enum) == 6
    att = re.search(r"#define CLM_TF_STAGE_ATTENTION\(i\) \((\d+) \+ (\d+) \* \(i\)\)", hdr)
    lay = re.search(r"#define CLM_TF_STAGE_LAYER\(i\) \((\d+) \+ (\d+) \* \(i\)\)", hdr)
    assert (int(att[1]), int(att[2])) == (T._STOP_ATTENTION0, T._STOP_PER_LAYER)
    assert (int(lay[1]), int(lay[2])) == (T._STOP_LAYER0, T._STOP_PER_LAYER)
