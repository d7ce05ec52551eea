"""Numpy reference of the engine's per-read attention summary and peaks (include/chimeralm_hip.h, `clm_attn_summary`), written from
the definition and used by the tests of csrc/attn_weights.hip:

    n_pad   = length of the leading run of token id 4 ([PAD]);  has_sep = the last token is id 1 ([SEP])
    bases   = the positions in between;  masses = weight on the pads / on [SEP] / on the bases
    peaks   = the min(top_k, n_bases) bases of largest weight, descending, equal weights by lower position; positions are
              0-based among the bases.  A row with a non-finite weight has no peaks and NaN masses.

Without ties the peaks are notebooks/attention.ipynb's `np.argsort(weights)[-top_k:][::-1]` on the read's bases.
"""
from __future__ import annotations

import numpy as np

PAD_ID, SEP_ID = 4, 1


def softmax64(scores: np.ndarray) -> np.ndarray:
    s = np.asarray(scores, dtype=np.float64)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def summarize(weights: np.ndarray, ids: np.ndarray, top_k: int) -> dict:
    """One read: `weights` [L] as the kernel wrote them, `ids` [L]."""
    w = np.asarray(weights)
    ids = np.asarray(ids)
    L = len(ids)
    not_pad = np.flatnonzero(ids != PAD_ID)
    n_pad = int(not_pad[0]) if len(not_pad) else L
    has_sep = int(ids[-1] == SEP_ID)
    n_bases = max(0, L - n_pad - has_sep)
    out = {"n_pad": n_pad, "n_bases": n_bases, "has_sep": has_sep}
    if not np.isfinite(w).all():
        out.update(n_peaks=0, pos=[], weight=[], pad_weight=np.nan, sep_weight=np.nan, base_weight=np.nan)
        return out
    bases = w[n_pad: n_pad + n_bases]
    order = np.lexsort((np.arange(n_bases), -bases.astype(np.float64)))       # by descending weight, then ascending position
    n_peaks = min(int(top_k), n_bases)
    w64 = w.astype(np.float64)
    out.update(n_peaks=n_peaks, pos=[int(p) for p in order[:n_peaks]], weight=[bases[p] for p in order[:n_peaks]],
               pad_weight=float(w64[:n_pad].sum()), sep_weight=float(w64[-1]) if has_sep else 0.0,
               base_weight=float(w64[n_pad: n_pad + n_bases].sum()))
    return out


def check_against(att, ids: np.ndarray, top_k: int, rel: float = 1e-5) -> None:
    """An `engine.AttentionOutput` of HOST tensors with weights against `summarize` of those same weights: integer fields and
    peaks exactly, masses within `rel` of the fp64 sums."""
    f = {k: v.numpy() for k, v in att.fields().items()}
    w, pos, pw = att.weights.numpy(), att.peak_pos.numpy(), att.peak_weight.numpy()
    for b in range(len(ids)):
        r = summarize(w[b], ids[b], top_k)
        got = {k: int(f[k][b]) for k in ("n_pad", "n_bases", "has_sep", "n_peaks")}
        assert got == {k: r[k] for k in got}, (b, got, r)
        n = r["n_peaks"]
        assert pos[b, :n].tolist() == r["pos"], (b, pos[b].tolist(), r["pos"])
        assert pw[b, :n].tolist() == [float(x) for x in r["weight"]], b
        assert (pos[b, n:] == -1).all() and (pw[b, n:] == 0).all(), b
        assert all(0 <= p < r["n_bases"] for p in pos[b, :n]), b
        for k in ("pad_weight", "sep_weight", "base_weight"):
            assert abs(float(f[k][b]) - r[k]) <= rel * abs(r[k]), (b, k, float(f[k][b]), r[k])
