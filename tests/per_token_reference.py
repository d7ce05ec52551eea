"""Per-token comparison of the Hyena residual stream and pooling scores with the fp64 oracle (test infrastructure: host only, it
imports the oracle and nothing of the product).

The logits are an attention-weighted mean over the whole read pushed through a small head: an error confined to one token of
8,193 moves them by that token's attention weight times the error, far below any logit gate.  Here every token is judged by itself:

  truth(ids, sd)        the oracle's float64 forward: the residual rows behind every block and the pooling scores
  token_error(got, ref) [B, L]: max_c |got - ref| / max_c |ref[b, t, :]| -- per token, because the stream's scale grows with the
                        read length (largest row ~16 at 129 tokens, ~155 at 8,193) and one global scale would hide small rows
  yardstick(ids, sd)    the same statistics for the reference's own arithmetic -- the oracle's float32 forward -- against truth
  assert_per_token(...) everything finite; per read, max and rms over tokens of the error <= K x the yardstick's same statistic

A yardstick may also come from another model of the arithmetic (tests/error_model.py for the 16-bit modes): `Yardstick` holds
nothing but per-token errors.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from oracle import hyena_oracle as ho

SEG_LEN = 8192                      # tokens per segment of the long-read convolution (csrc/clm_common.h)
LAST_BLOCK = ho.N_LAYER - 1


@dataclass(frozen=True)
class Truth:
    """float64 rows of one batch: blocks[i] [B, L, 256] = the residual stream behind block i (blocks[3]: in front of ln_f),
    scores [B, L]"""
    blocks: tuple
    scores: np.ndarray

    @property
    def hidden(self) -> np.ndarray:
        return self.blocks[LAST_BLOCK]


@dataclass(frozen=True)
class Yardstick:
    """Per-token errors of a reference arithmetic against the truth: hidden [B, L] (normalised per token, of block `block`),
    scores [B, L] (absolute), raw = max |hidden - truth| un-normalised"""
    hidden: np.ndarray
    scores: np.ndarray
    raw: float
    block: int = LAST_BLOCK


def _trace_rows(trace) -> Truth:
    return Truth(tuple(trace[f"l{i}.out"].double().numpy() for i in range(ho.N_LAYER)), trace["scores"].double().numpy())


def truth(ids, sd) -> Truth:
    trace: dict = {}
    ho.forward(torch.as_tensor(np.asarray(ids).astype(np.int64)), sd, torch.float64, trace=trace)
    return _trace_rows(trace)


def token_error(got, ref64) -> np.ndarray:
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    return np.abs(got - ref64).max(axis=-1) / np.abs(ref64).max(axis=-1)


def yardstick_of(rows: Truth, ref: Truth, block: int = LAST_BLOCK) -> Yardstick:
    """The per-token errors of `rows` (any arithmetic's residual rows and scores) against `ref`"""
    return Yardstick(token_error(rows.blocks[block], ref.blocks[block]), np.abs(rows.scores - ref.scores),
                     float(np.abs(rows.blocks[block] - ref.blocks[block]).max()), block)


def yardstick(ids, sd, ref: Truth | None = None, block: int = LAST_BLOCK) -> Yardstick:
    trace: dict = {}
    ho.forward(torch.as_tensor(np.asarray(ids).astype(np.int64)), sd, torch.float32, trace=trace)
    return yardstick_of(_trace_rows(trace), truth(ids, sd) if ref is None else ref, block)


def stats(err: np.ndarray, keep: np.ndarray | None = None) -> tuple[float, float]:
    """(max, rms) over the kept tokens of one read"""
    e = err if keep is None else err[keep]
    return float(e.max()), float(np.sqrt(np.mean(e * e)))


def where(b: int, t: int, L: int) -> str:
    """The code path a token belongs to, for a failure message"""
    return (f"(b={b}, t={t}) of {L}: 128-token tile {t // 128}, t % 64 = {t % 64}, t % 128 = {t % 128}, segment {t // SEG_LEN}"
            f"{', the last token' if t == L - 1 else ''}")


def position_classes(L: int) -> dict[str, np.ndarray]:
    """The positions a tile kernel treats apart: tokens 0-1 of every 128-token tile (the gated hand-over's history and patch path),
    the read's last token (peeled, or aliased in an L = N/2 + 1 transform), the first token of every 8192-token segment"""
    t = np.arange(L)
    return {"tokens 0-1 of a 128-token tile": t % 128 < 2, "the last token": t == L - 1, "the first token of a segment": t % SEG_LEN == 0}


def ratios(got_h, got_s, ref: Truth, yard: Yardstick, rows=None) -> dict[str, float]:
    """Worst ratio over the reads of engine statistic / yardstick statistic: hidden and scores, max and rms"""
    eh, es = token_error(got_h, ref.blocks[yard.block]), np.abs(np.asarray(got_s, dtype=np.float64) - ref.scores)
    out = {"h_max": 0.0, "h_rms": 0.0, "s_max": 0.0, "s_rms": 0.0}
    for b in range(eh.shape[0]):
        keep = None if rows is None else rows[b]
        for name, e, y, k in (("h", eh[b], yard.hidden[b], keep), ("s", es[b], yard.scores[b], None)):
            (m, r), (ym, yr) = stats(e, k), stats(y, k)
            out[name + "_max"] = max(out[name + "_max"], m / ym)
            out[name + "_rms"] = max(out[name + "_rms"], r / yr)
    return out


def assert_per_token(got_h, got_s, ids, sd, K, rows=None, *, ref: Truth | None = None, yard: Yardstick | None = None, classes=False):
    """got_h [B, L, 256] against the truth's rows of block `yard.block` (the last one unless the yardstick says otherwise), got_s
    [B, L] against its scores.  rows: bool [B, L], the tokens whose hidden rows are compared (None: all); the scores of every token
    always are.  ref / yard: computed here when not handed in (the float32 oracle is the default yardstick).  classes: also hold
    each position class (position_classes) to the line of all tokens, naming the class that breaks it."""
    ids = np.asarray(ids)
    B, L = ids.shape
    got_h, got_s = np.asarray(got_h), np.asarray(got_s)
    assert got_h.shape == (B, L, ho.D_MODEL) and got_s.shape == (B, L), (got_h.shape, got_s.shape)
    ref = truth(ids, sd) if ref is None else ref
    yard = yardstick(ids, sd, ref) if yard is None else yard
    keep_all = np.ones((B, L), bool) if rows is None else np.asarray(rows, bool)
    assert keep_all.shape == (B, L) and keep_all.any(axis=1).all()
    assert np.isfinite(got_h[keep_all]).all(), "hidden rows: not finite at " + where(*np.argwhere(~np.isfinite(got_h).all(-1) & keep_all)[0], L)
    assert np.isfinite(got_s).all(), "scores: not finite at " + where(*np.argwhere(~np.isfinite(got_s))[0], L)
    eh = token_error(np.where(keep_all[..., None], got_h, ref.blocks[yard.block]), ref.blocks[yard.block])
    es = np.abs(got_s.astype(np.float64) - ref.scores)
    for b in range(B):
        for name, e, y, keep in ((f"hidden rows (block {yard.block})", eh[b], yard.hidden[b], keep_all[b]),
                                 ("scores", es[b], yard.scores[b], np.ones(L, bool))):
            (ymax, yrms), (emax, erms) = stats(y, keep), stats(e, keep)
            worst = int(np.argmax(np.where(keep, e, -1.0)))
            if classes:
                for cname, sel in position_classes(L).items():
                    sel = sel & keep
                    if sel.any():
                        tc = int(np.argmax(np.where(sel, e, -1.0)))
                        assert e[tc] <= K * ymax, (f"{name}, {cname}: error {e[tc]:.3e} at {where(b, tc, L)} > {K} x {ymax:.3e} "
                                                  f"(the yardstick's maximum over all tokens of the read)")
            assert emax <= K * ymax, (f"{name}: max error {emax:.3e} at {where(b, worst, L)} > {K} x {ymax:.3e} "
                                      f"(ratio {emax / ymax:.3g})")
            assert erms <= K * yrms, (f"{name}, read {b}: rms error {erms:.3e} > {K} x {yrms:.3e} (ratio {erms / yrms:.3g}); "
                                      f"worst token {where(b, worst, L)}: {emax:.3e}")
