"""CPU: the reference, the yardstick, a second evaluation and planted defects of the row-wise gate of DNAConvNet's training kernels
(tests/cnn_train_rows.py; the engine's side is tests/test_gpu_cnn_train_rows.py).

(a) The EXPLICIT backward of `cnn_train_rows.evaluate` equals autograd over tests/cnn_train_reference.py's forward in float64 to 1e-12
    of every tensor's maximum (db_i, 0 in exact arithmetic, against dbeta_i's).
(b) CEILING.  For every case of the GPU file and every output the float32 yardstick stays below 1e-4 at EVERY row, so that K x
    yardstick is never a loose bound.  (With the cdf taken as 0.5 (1 + erf) the odd channels under `dead` read 3.4e-2 in dg, dbeta and
    dW; `cnn_train_rows._cdf` and the kernels take it as 0.5 erfc.)
(c) A SECOND float32 evaluation (a library convolution; column sums, dW and dT per 1,000 positions) stays within 32 x the yardstick
    per read, max and rms over rows.
(d) THE CHOICE condition of cnn_train_rows.choice_report holds for the yardstick's own choice with K = 2 (its two candidates are
    each off by at most the channel's largest error), and at most 0.05 % of a block's windows differ from float64's.
(e) `ct_split`, restated in Python, gives the chunks and grids the cases were chosen for; a change of the kernel file's constants
    fails here first (the constants are read from csrc/cnn_train.hip).
(f) PLANTED DEFECTS, each in the float32 evaluation, never in the engine: the row gate must see every one (a row above
    max(16 x yardstick, 32 x 2^-24)); the verdict of the tensor-wide gate of tests/test_gpu_cnn_train.py on the same tensors is
    printed and asserted as measured (PLANTED's last column; DESIGN.md 5.16b has the table).  It is blind to `small_row`: under
    dpooled x 2^-(c mod 13) and BatchNorm weights x 2^-(c mod 13) the dW_2 rows of the channels c mod 13 = 12 are 2^-24 of the largest
    row, and losing a whole tap of them moves nothing tensor-wide.  It sees the other ten: each is gross where it strikes (a
    full-size term at a few positions), and largest error over largest entry notices that.  There tests/test_gpu_cnn_train.py lacks
    not the formula but the inputs: its shapes never reach `last_chunk` and `dt_stale`, its ids need not hold a once-seen token, and it
    has no channel whose variance is below eps.
"""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

import cnn_train_reference as ctr
import cnn_train_rows as R
import grad_rows as G

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", [R.SHAPES[1] + R.PLAIN, R.SHAPES[2] + ("channels", "drop", "gamma")], ids=R.case_id)
def test_explicit_backward_is_autograd(case):
    seed, B, L = case[:3]
    ids, params, keeps, _, _ = R.make_inputs(case)
    sd = dict(R._state_dict(seed))
    sd.update(zip(ctr.PARAM_KEYS[:13], params))
    p_drop = 0.0 if keeps is None else 0.1
    ref = ctr.cnn_train_reference(sd, ids, ctr.synthetic_labels(seed, B), torch.float64, keep=keeps, p_drop=p_drop)
    ev = R.evaluate((ids, params, keeps, 1.0 / (1.0 - p_drop), ref["dpooled"]), torch.float64, choice=ref["choice"])
    pairs = [("pooled", ev["pooled"], ref["pooled"], None)]
    for i in range(3):
        pairs += [(f"{k}{i}", ev[f"{k}{i}"], ref[k][i], None) for k in ("z", "y", "mean", "var", "dz")]
    for k, key in zip(R.GRAD_KEYS, ctr.PARAM_KEYS):
        scale = ref["grads"][key.replace("0.bias", "1.bias")] if k.startswith("db") and not k.startswith("dbeta") else None
        pairs.append((k, ev[k], ref["grads"][key], scale))
    for name, a, b, scale in pairs:
        err = float((a - b).abs().max() / (b if scale is None else scale).abs().max())
        print(f"{R.case_id(case)} {name}: {err:.2e}")
        assert err <= 1e-12, name


# ------------------------------------------------------------------------------------------------------------- (b), (c), (d)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_yardstick(case):
    L = case[2]
    inp, r64, r32 = R.host_case(case)
    tag = f"cnn {R.case_id(case)}"
    yard = R.rows(r32, r64, L)
    G.ceiling(tag, yard)
    G.second(tag, R.rows(R.evaluate(inp, torch.float32, choice=r32["choice"], second=True), r64, L), yard)
    report = R.choice_report(r32["choice"], r64, r32, 2, L)
    print("\n".join(R.choice_lines(tag, report)))
    assert R.choice_ok(report)


def test_profiles_are_powers_of_two():
    for prof in ("gamma", "convrows"):
        plain, shaped = R.make_params(2, "plain"), R.make_params(2, prof)
        for a, b in zip(plain, shaped):
            f = (b / a)[a != 0]
            assert bool((torch.frexp(f)[0] == 0.5).all()) and float(f.min()) >= 2.0 ** -12, prof
    ids = R.make_ids(2, 3, 203, 17)
    assert int((ids == 0).sum()) == 1 and int(ids[0, 0]) == 0 and int((ids == 1).sum()) == 1 and int(ids[2, 202]) == 1
    keeps, scale = R.make_keeps(2, 3, 203, "rows3")
    assert scale == 1.0 and bool(keeps[0].all()) and bool(keeps[1].all()) and bool(keeps[2].all())       # L_3 = 3: a mask of ones
    keeps, _ = R.make_keeps(3, 2, 1031, "rows3")
    assert keeps[2][0, :, 0].nonzero().flatten().tolist() == [0, 8, 15] and bool(keeps[0].all()) and bool(keeps[1].all())
    assert sum(c[5] == "rows3" and c[2] >= 1031 for c in R.CASES) == 2


# ------------------------------------------------------------------------------------------------------------- (e)
def test_ct_split_gives_the_grids_the_cases_were_chosen_for():
    src = (REPO / "chimeralm_amd" / "csrc" / "cnn_train.hip").read_text()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))          # noqa: E731
    assert (const("CT_STAT_GRID"), const("CT_DT_GRID"), const("CT_DW_GRID"), const("CT_DT_SUB"), const("CT_SLICES")) == \
        (R.STAT_GRID, R.DT_GRID, R.DW_GRID, R.DT_SUB, R.SLICES)
    mins = [int(m) for m in re.findall(r"ct_split\(\w+, CT_\w+_GRID, (\d+), chunk, grid\);", src)]
    assert mins == [R.STAT_MIN, R.DY_MIN, R.DT_MIN]
    n = 2 * 16421
    assert n == 32842
    assert R.ct_split(n, R.STAT_GRID, R.STAT_MIN) == (65, 506) and n - 505 * 65 == 17            # stats: the last workgroup has 17 rows
    assert R.ct_split(2 * (16421 // 4), R.STAT_GRID, R.DY_MIN) == (17, 483)                      # dy over the B L_1 pooled rows
    assert R.ct_split(n, R.DT_GRID, R.DT_MIN) == (129, 255)
    assert R.slices(506) == [127, 127, 127, 125] and R.slices(255) == [64, 64, 64, 63]           # the uneven four slices
    n = 2 * 65540
    assert n == 131080
    assert R.ct_split(n, R.DT_GRID, R.DT_MIN) == (513, 256) and 513 - R.DT_SUB == 1              # a second stretch of one position
    assert R.ct_split(n, R.STAT_GRID, R.STAT_MIN) == (257, 511)
    assert 2 * (65540 // 4) == 32770 and R.ct_split(32770, R.STAT_GRID, R.STAT_MIN) == (65, 505)  # block 1 is capped too
    tiles = 2 * -(-(65540 // 4) // 64)
    assert sorted({len(range(g, tiles, R.DW_GRID)) for g in range(R.DW_GRID)}) == [14, 15]       # dw: tiles per workgroup
    assert 5 * -(-(2053 // 4) // 64) == 45 > R.DW_GRID
    # below the cap nothing of this is reached: the largest case of tests/test_gpu_cnn_train.py
    assert R.ct_split(8 * 2055, R.STAT_GRID, R.STAT_MIN) == (64, 257) and R.ct_split(8 * 2055, R.DT_GRID, R.DT_MIN) == (128, 129)


# ------------------------------------------------------------------------------------------------------------- (f)
PLANTED = [  # (defect, case, does the tensor-wide gate see it)
    ("small_row", R.SHAPES[2] + ("channels", "none", "gamma"), False),  # rows of size 2^-24 of the tensor's largest
    ("m_covered", R.SHAPES[1] + R.PLAIN, True),                        # m1, m2 over the 64 covered positions of 67
    ("dz_uncovered", R.SHAPES[1] + R.PLAIN, True),                     # dz = 0 at positions 64 .. 66
    ("dz_unchosen", R.SHAPES[2] + R.PLAIN, True),
    ("across_reads", R.SHAPES[2] + ("reads", "none", "plain"), True),  # read b + 1 is 2^-10 of read b
    ("last_chunk", R.SHAPES[5] + R.PLAIN, True),                       # 17 of 32,842 rows
    ("dt_stale", R.SHAPES[6] + R.PLAIN, True),                         # position 512 of each of the 256 chunks
    ("outside_counted", R.SHAPES[3] + R.PLAIN, True),
    ("once_lost", R.SHAPES[1] + R.PLAIN, True),
    ("no_eps", R.SHAPES[2] + ("uniform", "none", "convrows"), True),
    ("no_mask_scale", R.SHAPES[2] + ("uniform", "drop", "plain"), True),
]


@pytest.mark.parametrize("defect,case,old_sees", PLANTED, ids=[d for d, _, _ in PLANTED])
def test_planted(defect, case, old_sees):
    inp, r64, r32 = R.host_case(case)
    ev = R.evaluate(inp, torch.float32, choice=r32["choice"], defect=defect)
    seen = G.planted(f"cnn {defect} at {R.case_id(case)}", R.rows(ev, r64, case[2]), R.rows(r32, r64, case[2]), R.old_gates(ev, r64, r32))
    assert seen == old_sees, "the tensor-wide gate's verdict changed: update PLANTED and DESIGN.md 5.16b"
