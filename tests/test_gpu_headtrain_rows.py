"""GPU (MI355X): the head fine-tune's pooling kernels (csrc/pool_train.hip behind Engine.pool_forward / pool_backward) against
float64 ROW BY ROW.

tests/test_gpu_headtrain.py divides the largest error of a whole tensor by the tensor's largest entry on one kind of input (unit-normal
rows, the seeded head's weights): it holds the largest rows of dW1, db1 and dw2, and no case decides where the softmax mass sits.
Here every output is cut into rows with a denominator of their own (tests/grad_rows.py, the pooling section: the table, the profiles,
the cases), and the bound is, per read, for the max and the rms over rows,

    engine <= max(K x yardstick, 32 x 2^-24)        yardstick: the same formulas in float32 on the CPU, never the engine.

tests/test_headtrain_rows_host.py holds the yardstick below 1e-4 at every row of every case and shows what the gate does with planted
defects.  One token (1 x 1): the forward's rows are held; every gradient is 0 in exact arithmetic and is held to 32 x 2^-24 in
absolute terms, as tests/test_gpu_headtrain.py holds it (the forward's pooled and the backward's own ln_f need not agree to the bit).

BIT-EXACT RELATIONS: a second call gives identical bits; dpooled x 2^-20 gives 2^-20 x every gradient wherever the scaled value stays
above 2^-60 (ds is linear in dpooled and the scale is exact) -- SCALING_EXACT says what the first run showed.
At 257 x 3 the gradients of reads 0 .. 255 (beta = 0) plus read 256 (beta = 1) are held to the same rows as the one call.

CLM_HEADTRAIN_ROWS_PARITY=<file> appends every line and the RATIO summary (profiles/headtrain_rows_parity.txt is one run).

K, from the first run on the fixed kernel (no bound set before it; profiles/headtrain_rows_parity.txt is that run, 56 tests in 3.6 s):
the worst engine / yardstick ratio among figures above the floor, over the cases, reads and both statistics, per output:
    output   all figures   above the floor   engine max   yardstick max
    scores      134.08        -              2.82e-07     3.75e-07     (no row reaches the floor: the forward keeps gelu_erf)
    attn        132.62        6.24           2.15e-05     6.09e-05
    pooled        9.21        3.04           8.32e-06     1.26e-05
    dW1           2.04        2.04           1.50e-04     1.00e-04
    db1           3.77        3.10           1.46e-04     9.91e-05
    dw2           2.74        2.74           1.46e-04     9.97e-05
    db2           inf         1.36           3.52e-05     2.58e-05     (inf: a yardstick of exactly 0 below the floor)
(the two maxima columns include 1-65-b1_offsets+peak40@last, dW1 1.50e-4 against 1.00e-4: the case ran and was dropped afterwards for the host
file's ceiling, tests/grad_rows.py; the largest yardstick of the cases kept is 5.7e-5.)
K = the smallest power of two >= 2 x the worst ratio above the floor = 2 x 6.24 = 12.5 -> K = 16.  WHICH READING OF THE RULE: the literal
one, the 6.24 counted.  Set apart as an outlier it would leave 2 x 3.10 -> K = 8, under which the 6.24 row still passes on this
yardstick (1.97e-6 against max(8 x 3.2e-7, floor) = 2.5e-6) -- but by a margin of 1.28, and the float32 yardstick itself moves with the
CPU that computes it (attn of 3 x 200 b1_offsets+peak40@last: 2.9e-5 on one host, 5.7e-5 on another).  A three-token read's yardstick
a factor 1.3 lower would fail a correct kernel under K = 8.  16 is what the rule gives without a judgement call, and no other figure
comes within a factor 5 of it.  The 6.24 stands apart from the rest
(3.10 next) and is explained, not a defect: attn at 257 x 3 under peak8@last, engine 1.97e-6 -- at the floor's edge -- against that
read's yardstick of 3.2e-7.  An a_t's relative error is the absolute error of s_t - max (here |s| up to 8 x the plain scores), and a
read of three tokens gives the yardstick three draws: among 257 reads some yardstick is lucky.  The scores rows of the same case sit
at 1.3e-7 of their denominator.  Every other figure above the floor is at or below 3.10 x.

FOUND AND FIXED in csrc/pool_train.hip: pool_bwd_kernel took the normal cdf as 0.5 (1 + erf), a multiple of 2^-25.  Under b1_offsets,
on the parent's library (same run, the file's BEFORE section), engine against yardstick, max over the features of an offset:
    b1 - 8     dw2 0.95 - 1.00 (the row is lost)   db1 2.6e-2 - 2.8e-2   dW1 3.0e-2       yardstick 2.5e-6 - 3.7e-6
    b1 - 6     dw2 1.0e-2 - 5.2e-2                 db1 3.9e-4 - 1.8e-3   dW1 1.8e-3 - 8.5e-3
    b1 - 5.5   dw2 2.5e-3 - 2.0e-2                 db1 1.0e-4 - 8.1e-4   dW1 2.4e-4 - 2.3e-3
    b1 - 4.5   dw2 5.5e-5 - 1.5e-4                 db1 3.5e-6 - 9.0e-6   dW1 4.9e-6 - 2.8e-5   (not among the predicted classes; it fails in dw2)
worst ratios 463,413 (dw2), 15,718 (db1), 11,855 (dW1), while tests/test_gpu_headtrain.py passed.  With normal_cdf = 0.5 erfcf(-u / sqrt 2)
(csrc/clm_common.h, shared with cnn_train.hip) the same classes read 1.4e-6 - 7.5e-6 against yardsticks of 5.6e-7 - 3.7e-6; offsets
0, + 3, + 6 and - 3 read alike before and after.
SCALING: dpooled x 2^-20 gave 2^-20 x every gradient bit for bit at all four cases, no element differing (asserted).
"""
from __future__ import annotations

import os

import pytest
import torch

import grad_rows as G
import headtrain_reference as hr

pytestmark = pytest.mark.gpu

K = G.K["pool"]
SCALING_EXACT = True                                      # False: report only
SCALE, KEEP = 2.0 ** -20, 2.0 ** -60
_ratios: dict = {}


def _record(lines):
    print("\n".join(lines))
    if os.environ.get("CLM_HEADTRAIN_ROWS_PARITY"):
        with open(os.environ["CLM_HEADTRAIN_ROWS_PARITY"], "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def engine(built_lib):
    from chimeralm_amd.engine import Engine

    eng = Engine("cuda:0", precision="fp32", chunk_reads=4)
    eng.load_state_dict(G.pool_sd())
    yield eng
    eng.close()
    _record(G.summary(_ratios))


def _run(eng, c, reads=slice(None), dp_scale=1.0, out=None, beta=0.0) -> dict:
    """pool_forward + pool_backward on the engine, as tests/test_gpu_headtrain.py `_run` -> the keys of `grad_rows.pool_eval` (CPU);
    `attn` from the returned scores and statistics in float32, as pool_bwd_kernel takes it."""
    dev = eng.device
    rows = c["rows"][reads].contiguous().to(dev)
    w1, b1, w2, b2 = (c[k].to(dev).contiguous() for k in ("w1", "b1", "w2", "b2"))
    scores, stats, pooled = eng.pool_forward(rows, w1, b1, w2.view(-1), b2)
    grads = eng.pool_backward(rows, w1, b1, w2.view(-1), scores, stats, pooled, (c["dpooled"][reads] * dp_scale).contiguous().to(dev),
                              out=out, beta=beta)
    torch.cuda.synchronize()
    got = {"scores": scores.cpu(), "stats": stats.cpu(), "pooled": pooled.cpu()}
    got["attn"] = hr.attn_from(got["scores"], got["stats"])
    got.update({k: g.cpu().reshape(s) for k, g, s in zip(G.POOL_GRADS, grads, ((256, 256), (256,), (256,), ()))})
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    return got


def _hold(tag, got, r64, r32, L):
    eng_rows, yard_rows = G.pool_rows(got, r64, grads=L > 1), G.pool_rows(r32, r64, grads=L > 1)
    lines, bad, ratios = [], [], {}
    G.hold(tag, eng_rows, yard_rows, K, lines, bad, ratios)
    print("\n".join(lines))
    rms = lambda v: float(v.pow(2).mean().sqrt())                                    # noqa: E731
    _record([f"ROWS pool {tag:40s} {name:8s} engine max {G.worst(e):.2e} rms {rms(e):.2e}  yardstick max {G.worst(y):.2e} rms {rms(y):.2e}  "
             f"K {K}  worst ratio {ratios[name][0]:7.2f}  above the floor {ratios[name][1]:7.2f}"
             for (name, e, _), (_, y, _) in zip(eng_rows, yard_rows)])
    if "b1_offsets" in tag:                                # the features by their offset: what the cdf's form decides
        for (name, e, _), (_, y, _) in zip(eng_rows, yard_rows):
            if name in ("dW1", "db1", "dw2"):
                _record([f"CLASS pool {tag:40s} {name:8s} " + "  ".join(f"b1{G.POOL_OFFSETS[k]:+g}: {float(e[0, k::8].max()):.1e} / {float(y[0, k::8].max()):.1e}"
                                                                       for k in range(8)) + "   (engine / yardstick, max over the features f mod 8 = k)"])
    for name, v in ratios.items():
        r = _ratios.setdefault(name, [0.0, 0.0])
        r[0], r[1] = max(r[0], v[0]), max(r[1], v[1])
    if L == 1:
        for k in G.POOL_GRADS:
            worst = float(got[k].abs().max())
            _record([f"ROWS pool {tag:40s} {k:8s} one token: max |{k}| {worst:.3e}  floor {G.FLOOR:.3e}"])
            if not worst <= G.FLOOR:
                bad.append(f"{tag} max |{k}| {worst:.3e} above the floor")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", G.POOL_CASES, ids=G.case_id)
def test_rows(engine, case):
    inp, r64, r32 = G.pool_case(*case)
    _hold(G.case_id(case), _run(engine, inp), r64, r32, case[1])


SAME = [(3, 200, "b1_offsets+peak8@last"), (257, 3, "b1_offsets"), (5, 4097, "plain")]


@pytest.mark.parametrize("case", SAME, ids=G.case_id)
def test_second_call_is_identical(engine, case):
    inp = G.pool_inputs(*case)
    a, b = _run(engine, inp), _run(engine, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", [(1, 65, "plain"), (2, 130, "b1_offsets"), (3, 200, "peak8@last"), (257, 3, "plain")], ids=G.case_id)
def test_scales_exactly(engine, case):
    """dpooled x 2^-20: ds_t = a_t ((x_t - p) . dp) is linear in dp, every later step multiplies ds by forward values or adds such
    products, and the scale is an exact power of two: every gradient scales by exactly 2^-20 while nothing is subnormal."""
    inp = G.pool_inputs(*case)
    full, scaled = _run(engine, inp), _run(engine, inp, dp_scale=SCALE)
    for k in ("scores", "stats", "pooled"):
        assert torch.equal(full[k], scaled[k]), k
    ok = True
    for k in G.POOL_GRADS:
        keep = full[k].abs() * SCALE >= KEEP
        same = (scaled[k] * (1.0 / SCALE) == full[k]) | ~keep
        _record([f"SCALING pool {G.case_id(case)} {k}: {int(keep.sum())} of {keep.numel()} elements above 2^-60 after scaling, {int((~same).sum())} differ"])
        ok = ok and bool(same.all())
    if SCALING_EXACT:
        assert ok


@pytest.mark.parametrize("profile", ["plain", "b1_offsets"])
def test_last_read_accumulates(engine, profile):
    """257 x 3 in two calls: reads 0 .. 255 fill the 256-workgroup grid with one tile each (beta = 0), read 256 is added (beta = 1);
    in the one call workgroup 0 owns the tiles of reads 0 and 256.  Both are held to the same rows."""
    inp, r64, r32 = G.pool_case(257, 3, profile)
    out = tuple(torch.full(s, float("nan"), device=engine.device) for s in ((256, 256), (256,), (256,), (1,)))   # (beta = 0 does not read them)
    a = _run(engine, inp, reads=slice(0, 256), out=out, beta=0.0)
    b = _run(engine, inp, reads=slice(256, 257), out=out, beta=1.0)
    got = {k: torch.cat([a[k], b[k]]) for k in ("scores", "stats", "attn", "pooled")}
    got.update({k: b[k] for k in G.POOL_GRADS})
    _hold(f"257-3-{profile} in two calls", got, r64, r32, 3)
