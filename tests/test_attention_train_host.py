"""The training attention op's formulas and keep mask on the CPU (tests/attention_train_reference.py): the hand-written backward
against fp64 autograd, and the statistics of the mask's `bits`."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import attention_train_reference as R


@pytest.mark.parametrize("L", [1, 2, 33, 65, 130])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_hand_formulas_match_fp64_autograd(L, p):
    B = 2
    qkv, dout = R.make_qkv(B, L, "normal").double(), R.make_dout(B, L).double()
    keep = None if p == 0.0 else torch.from_numpy(R.keep_mask(11, B, L, p))
    hand, auto = R.backward(qkv, keep, p, dout), R.autograd(qkv, keep, p, dout)
    for k in ("out", "dq", "dk", "dv"):
        assert float((hand[k] - auto[k]).abs().max()) <= 1e-12, k
    q, k = R.heads(qkv[..., :256]), R.heads(qkv[..., 256:512])
    lse = torch.logsumexp(q @ k.transpose(-1, -2) / math.sqrt(32.0), dim=-1)
    assert float((hand["lse"] - lse).abs().max()) <= 1e-12
    # delta_i = sum_j p_ij dS'_ij holds with dropout: the rows of dS sum to zero only without it, but dS itself is autograd's
    if p == 0.0:
        assert R.forward(qkv, None, 0.0)[2].sum(dim=-1).sub(1.0).abs().max() <= 1e-12


def _within(rate: float, want: float, n: int) -> bool:
    sigma = math.sqrt(want * (1.0 - want) / n)
    print(f"rate {rate:.6f} want {want:.6f} sigma {sigma:.2e} -> {(rate - want) / sigma:+.2f} sigma")
    return abs(rate - want) <= 5.0 * sigma


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15, 12345678901234567])
def test_mask_quality(p, seed):
    """2^20 draws (2 reads x 8 heads x 256 x 256): the keep rate, and the agreement of neighbouring rows, columns, heads and seeds
    against p^2 + (1 - p)^2, each within 5 binomial sigma."""
    B, L = 2, 256
    a = R.keep_mask(seed, B, L, p)
    assert a.size == 1 << 20
    thr = R.threshold(p)
    keep_rate = 1.0 - thr / 2.0 ** 32
    assert _within(a.mean(), keep_rate, a.size)
    agree = keep_rate ** 2 + (1.0 - keep_rate) ** 2
    rows, cols = a[:, :, 1:] == a[:, :, :-1], a[..., 1:] == a[..., :-1]
    flat = a.reshape(B * 8, L, L)
    hd = flat[1:] == flat[:-1]
    sd = a == R.keep_mask((seed + 1) & ((1 << 64) - 1), B, L, p)
    for name, eq in (("rows", rows), ("columns", cols), ("heads", hd), ("seeds", sd)):
        assert _within(eq.mean(), agree, eq.size), name


def test_mask_edges():
    assert R.keep_mask(5, 1, 65, 0.0).all()                         # p = 0 keeps everything
    assert R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 31
    assert R.threshold(0.1) == int(np.float32(0.1).astype(np.float64) * 2 ** 32 + 0.5)
    # a pure function of (seed, b * 8 + h, i, j): read 1 of a batch is read 0 of a batch that starts at b0 = 1; the top-left corner
    # of a longer read is the shorter read
    a = R.keep_mask(9, 3, 40, 0.3)
    assert np.array_equal(a[1:2], R.keep_mask(9, 1, 40, 0.3, b0=1))
    assert np.array_equal(a[:, :, :17, :17], R.keep_mask(9, 3, 17, 0.3))
    assert not np.array_equal(R.keep_mask(9, 1, 40, 0.3), R.keep_mask(9 + (1 << 32), 1, 40, 0.3))   # the high seed word counts
