"""CPU: the yardstick, a second evaluation and planted defects of the row-wise gate of the head fine-tune's pooling kernels
(tests/grad_rows.py's pooling section over tests/headtrain_reference.py; the engine's side is tests/test_gpu_headtrain_rows.py).

(a) CEILING.  For every case of the GPU file and every output the float32 yardstick stays below 1e-4 at EVERY row, so that K x
    yardstick is never a loose bound.  (With the cdf taken as 0.5 (1 + erf) the features under b1 - 8 read 0.98 in dw2 and 3e-2 in dW1
    and db1; `headtrain_reference.cdf` and, since this file exists, pool_bwd_kernel take it as 0.5 erfc.)
(b) A SECOND float32 evaluation, every sum over tokens taken in mirrored order, stays within 32 x the yardstick per read, max and
    rms over rows.
(c) The profiles scale by exact powers of two, and `peak` puts the largest softmax weight where it says (its share of the mass, 0.17 - 0.99, is printed).
(d) PLANTED DEFECTS, eight (`headtrain_reference.DEFECTS`; the ragged tile under two inputs), each in the float32 evaluation, never
    in the engine.  The row gate's verdict (a row above max(16 x yardstick, 32 x 2^-24)) and the verdict of the tensor-wide gate of tests/test_gpu_headtrain.py on the same tensors are both asserted as
    measured (PLANTED's last two columns; DESIGN.md 5.16c has the table).
"""
from __future__ import annotations

import pytest
import torch

import grad_rows as G
import headtrain_reference as hr


def _rows(ev, r64, L):
    return G.pool_rows(ev, r64, grads=L > 1)


# ------------------------------------------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("case", G.POOL_CASES, ids=G.case_id)
def test_yardstick(case):
    B, L, _ = case
    inp, r64, r32 = G.pool_case(*case)
    tag = f"pool {G.case_id(case)}"
    yard = _rows(r32, r64, L)
    G.ceiling(tag, yard)
    G.second(tag, _rows(G.pool_eval(inp, torch.float32, reverse=True), r64, L), yard)
    if L == 1:                                             # one token: softmax weight 1, every gradient exactly 0 in both precisions
        for r in (r64, r32):
            assert all(float(r[k].abs().max()) == 0.0 for k in G.POOL_GRADS)
            assert all(float(r["den"][k].abs().max()) == 0.0 for k in G.POOL_GRADS)


# ------------------------------------------------------------------------------------------------------------- (c)
def test_profiles():
    plain = G.pool_inputs(3, 200, "plain")
    for prof, key, least in (("w2_ramp", "w2", 2.0 ** -12), ("w1_rows", "w1", 2.0 ** -10), ("dp_channels", "dpooled", 2.0 ** -12), ("peak8@last", "w2", 8.0)):
        f = (G.pool_inputs(3, 200, prof)[key] / plain[key])[plain[key] != 0]
        assert bool((torch.frexp(f)[0] == 0.5).all()) and float(f.min()) == least, prof
    # (x 40 = 5 x 2^3 rounds each w2 once, in the input: every evaluation and the engine read the same rounded fp32 values)
    assert torch.equal(G.pool_inputs(3, 200, "peak40@first")["w2"], plain["w2"] * 40.0)
    off = G.pool_inputs(3, 200, "b1_offsets")["b1"] - plain["b1"]
    assert float((off - torch.tensor(G.POOL_OFFSETS)[torch.arange(256) % 8]).abs().max()) <= 2.0 ** -20      # (the sum rounds once, in the input)
    for B, L in ((1, 65), (3, 200), (2, 130)):
        for at, pos in (("first", 0), ("last", L - 1), ("tile", (L - 1) // 64 * 64)):
            for scale in (8, 40):                          # (the mass is printed, not held: 0.17 to 0.99 of it at x 8 and x 40 on these rows)
                inp, r64, _ = G.pool_case(B, L, f"peak{scale}@{at}")
                a = r64["attn"]
                print(f"peak{scale}@{at} {B} x {L}: softmax mass at token {pos}: {a[:, pos].tolist()}")
                assert bool((a.argmax(1) == pos).all())
                assert sorted(inp["rows"].flatten().tolist()) == sorted(G.pool_inputs(B, L, "plain")["rows"].flatten().tolist())


# ------------------------------------------------------------------------------------------------------------- (d)
PLANTED = [  # (defect, case, the row gate sees it, the tensor-wide gate sees it)
    ("cdf_erf", (1, 65, "b1_offsets"), True, False),
    ("cdf_erf", (3, 200, "b1_offsets"), True, False),
    ("last_tile", (1, 65, "plain"), True, True),
    ("last_tile", (2, 130, "plain"), True, True),
    ("last_tile", (3, 200, "plain"), True, True),
    ("last_tile", (3, 200, "peak40@last"), True, True),
    ("no_p", (3, 200, "plain"), True, True),
    ("no_updf", (3, 200, "plain"), True, True),
    ("stats0", (3, 200, "plain"), True, True),
    ("w2_missing", (3, 200, "w2_ramp"), True, True),
    ("x_nobias", (3, 200, "plain"), True, True),
    ("stale_read", (257, 3, "plain"), True, True),
]


@pytest.mark.parametrize("defect,case,row_sees,old_sees", PLANTED, ids=[f"{d}-{G.case_id(c)}" for d, c, _, _ in PLANTED])
def test_planted(defect, case, row_sees, old_sees):
    assert defect in hr.DEFECTS
    inp, r64, r32 = G.pool_case(*case)
    ev = G.pool_eval(inp, torch.float32, defect=defect)
    seen = G.planted(f"pool {defect} at {G.case_id(case)}", _rows(ev, r64, case[1]), _rows(r32, r64, case[1]),
                     G.pool_old_gates(ev, r64, r32), expect_seen=row_sees)
    assert seen == old_sees, "the tensor-wide gate's verdict changed: update PLANTED and DESIGN.md 5.16c"
