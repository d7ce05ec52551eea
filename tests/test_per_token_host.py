"""Host: the per-token comparator (tests/per_token_reference.py) itself -- its yardstick is a stable line, and it sees errors the
logit gates do not: one token's row off by 1e-3 of its norm leaves the logits inside the parity gate (tests/test_gpu_parity.py
GATE) and fails here by two orders of magnitude, naming the token."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import per_token_reference as ptr
from oracle import hyena_oracle as ho

GATE = 1e-3                         # the parity gate on the logits (tests/test_gpu_parity.py)
K = 16                              # the cap the GPU tests may not exceed (tests/test_gpu_per_token.py)


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0, head_scale=3.0)


def _ids(B, L, seed, pads=3):
    ids, _ = ho.synthetic_batch(seed, B, L - 1, seed=99)
    ids[:, :pads] = 4
    return ids


@pytest.fixture(scope="module")
def batch(sd):
    """2 x 2,049 tokens: ids, truth, the float32 oracle's rows and scores, its yardstick"""
    ids = _ids(2, 2049, 5)
    ref = ptr.truth(ids, sd)
    trace: dict = {}
    ho.forward(torch.from_numpy(ids.astype(np.int64)), sd, torch.float32, trace=trace)
    rows32 = ptr._trace_rows(trace)
    return ids, ref, rows32, ptr.yardstick_of(rows32, ref)


@pytest.mark.parametrize("L", [129, 257, 2049])
def test_the_yardstick_is_stable_over_ids(sd, L):
    """Three draws of the ids per length: the worst token's error of the float32 oracle varies by less than 2x (hidden rows and
    scores), so K times it is a line and not a lottery."""
    worst_h, worst_s = [], []
    for seed in (5, 6, 7):
        y = ptr.yardstick(_ids(2, L, seed), sd)
        worst_h.append(float(y.hidden.max()))
        worst_s.append(float(y.scores.max()))
    print(f"L {L}: float32 oracle, worst token over three ids draws: hidden {worst_h}, scores {worst_s}")
    assert max(worst_h) < 2 * min(worst_h), worst_h
    assert max(worst_s) < 2 * min(worst_s), worst_s


def test_the_reference_passes_its_own_line(sd, batch):
    ids, ref, rows32, yard = batch
    ptr.assert_per_token(rows32.hidden, rows32.scores, ids, sd, 1, ref=ref, yard=yard, classes=True)
    ptr.assert_per_token(rows32.hidden, rows32.scores, ids, sd, K)              # (truth and yardstick computed inside)


@pytest.mark.parametrize("t", [0, 2048, 128])
def test_one_corrupted_token_fails_here_and_passes_the_logit_gate(sd, batch, t):
    """THE GAP: one token's row (first, last, first of tile 1) moved by 1e-3 of its norm in a random direction."""
    ids, ref, rows32, yard = batch
    b = 1
    bad = rows32.hidden.copy()
    d = np.random.default_rng(t).standard_normal(ho.D_MODEL)
    bad[b, t] += 1e-3 * np.linalg.norm(bad[b, t]) * d / np.linalg.norm(d)
    with pytest.raises(AssertionError, match=rf"hidden rows.*\(b={b}, t={t}\) of 2049"):
        ptr.assert_per_token(bad, rows32.scores, ids, sd, K, ref=ref, yard=yard)
    with torch.no_grad():
        hid = ho._ln(torch.from_numpy(bad).float(), sd, ho.BB + "ln_f", torch.float32)
        logits = ho.head_forward(hid, sd)
        want = ho.head_forward(ho._ln(torch.from_numpy(ref.hidden), sd, ho.BB + "ln_f", torch.float64), sd, torch.float64)
    err = float((logits.double() - want).abs().max())
    print(f"token {t} off by 1e-3 of its norm: per-token error {ptr.token_error(bad, ref.hidden)[b, t]:.2e} "
          f"(line: {K} x {yard.hidden[b].max():.2e}), logits off by {err:.2e}")
    assert err <= GATE


def test_a_corrupted_score_is_named(sd, batch):
    ids, ref, rows32, yard = batch
    s = rows32.scores.copy()
    s[0, 777] += 1e-2
    with pytest.raises(AssertionError, match=r"scores.*\(b=0, t=777\)"):
        ptr.assert_per_token(rows32.hidden, s, ids, sd, K, ref=ref, yard=yard)


def test_shifted_and_swapped_rows_fail(sd, batch):
    """Rows shifted by one token; a read swapped with its pair partner of the packed transform."""
    ids, ref, rows32, yard = batch
    with pytest.raises(AssertionError, match="hidden rows"):
        ptr.assert_per_token(np.roll(rows32.hidden, 1, axis=1), rows32.scores, ids, sd, K, ref=ref, yard=yard)
    with pytest.raises(AssertionError, match="scores"):
        ptr.assert_per_token(rows32.hidden, np.roll(rows32.scores, 1, axis=1), ids, sd, K, ref=ref, yard=yard)
    with pytest.raises(AssertionError, match="hidden rows"):
        ptr.assert_per_token(rows32.hidden[::-1], rows32.scores[::-1], ids, sd, K, ref=ref, yard=yard)


def test_rows_left_out_are_not_read_and_scores_always_are(sd, batch):
    ids, ref, rows32, yard = batch
    keep = np.ones(ids.shape, bool)
    keep[1, :128] = False
    junk = rows32.hidden.copy()
    junk[1, :128] = np.nan
    ptr.assert_per_token(junk, rows32.scores, ids, sd, K, rows=keep, ref=ref, yard=yard)
    with pytest.raises(AssertionError, match="not finite"):
        ptr.assert_per_token(junk, rows32.scores, ids, sd, K, ref=ref, yard=yard)
    s = rows32.scores.copy()
    s[1, 5] = np.nan
    with pytest.raises(AssertionError, match="scores: not finite"):
        ptr.assert_per_token(rows32.hidden, s, ids, sd, K, rows=keep, ref=ref, yard=yard)


def test_position_classes_name_the_class(sd, batch):
    """An error at token 1 of a tile that breaks the line is reported under its position class."""
    ids, ref, rows32, yard = batch
    bad = rows32.hidden.copy()
    bad[0, 1281] *= 1.0 + 1e-3                                   # token 1 of tile 10
    with pytest.raises(AssertionError, match=r"tokens 0-1 of a 128-token tile.*\(b=0, t=1281\)"):
        ptr.assert_per_token(bad, rows32.scores, ids, sd, K, ref=ref, yard=yard, classes=True)


def test_the_error_model_traces_the_same_rows_as_the_oracle(sd):
    """tests/error_model.py with no rounding switched on IS the float64 oracle, block by block; its 16-bit configurations move
    every token (no token is left exact but the documented ones)."""
    import error_model as em

    ids = _ids(2, 257, 5)
    ref = ptr.truth(ids, sd)
    trace: dict = {}
    with torch.no_grad():
        em.forward(ids.astype(np.int64), sd, {}, trace=trace)
    rows = ptr._trace_rows(trace)
    for i in range(ho.N_LAYER):
        assert np.abs(rows.blocks[i] - ref.blocks[i]).max() <= 1e-12 * np.abs(ref.blocks[i]).max()
    assert np.abs(rows.scores - ref.scores).max() <= 1e-12
    for mode, lo, hi in (("fp16", 1e-4, 1e-2), ("bf16", 1e-3, 1e-1), ("fp16c", 1e-5, 1e-2)):
        trace = {}
        with torch.no_grad():
            em.forward(ids.astype(np.int64), sd, em.ENGINE_MODES[mode], trace=trace)
        y = ptr.yardstick_of(ptr._trace_rows(trace), ref)
        print(f"{mode} model at 2 x 257: hidden max {y.hidden.max():.2e} rms {np.sqrt((y.hidden ** 2).mean()):.2e}, scores max {y.scores.max():.2e}")
        assert lo < y.hidden.max() < hi and (y.hidden > 0).all()
