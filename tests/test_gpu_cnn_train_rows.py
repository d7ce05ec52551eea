"""GPU (MI355X): DNAConvNet's training kernels (csrc/cnn_train.hip) against float64 ROW BY ROW, at the grids the workload runs.

tests/test_gpu_cnn_train.py runs whole steps through the loss and divides the largest error of a tensor by the tensor's largest entry:
it holds the largest rows, and its largest case (8 x 2,055) stays below the caps of `ct_split`.  Here the engine is driven directly
(`forward(ids, params, keeps, scale)`, `backward(gen, dpooled, params)`, `debug_fetch`), every output is cut into rows with a
denominator of their own (tests/cnn_train_rows.py: the table, the input profiles, the cases), and the bound is, per read, for the max
and the rms over rows,

    engine <= max(K x yardstick, 32 x 2^-24)        yardstick: the same formulas in float32 on the CPU, never the engine.

Both references are routed by the engine's own pooling choice, and the choice itself is held by `cnn_train_rows.choice_report`.
tests/test_cnn_train_rows_host.py holds the yardstick below 1e-4 at every row and shows what the gate does with planted defects.
A zero denominator demands an exact zero: d embedding of row 4 and of a token absent from the batch.

BIT-EXACT RELATIONS, asserted as such: a second identical forward + backward gives identical bits in all 13 gradients and in dz;
dpooled x 2^-20 gives 2^-20 x every gradient and dz wherever the scaled value stays above 2^-60 (SCALING_EXACT).

K, from the first run (no bound set before it; CLM_CNN_TRAIN_ROWS=<file> appends every line; profiles/cnn_train_rows_parity.txt is that
run, and its summary is the one place the table of worst ratios per output is kept): the worst engine / yardstick ratio among figures
above the floor, over the 38 cases, reads and both statistics, is 3.93 (dz2 at 3 x 203 under channels x drop x convrows);
K = the smallest power of two >= 2 x that ratio, capped at 16 -> K = 8.  46 tests in 18 s, the CPU references included.

FOUND AND FIXED in csrc/cnn_train.hip: the cdf of GELU and of its derivative was 0.5 (1 + erf), a multiple of 2^-25.  Under `dead`
(BatchNorm bias -6: u near -6, cdf 1e-9) y, dy and so dg, dbeta and dW of those channels were good to 3e-2 only, in the engine and in
any float32 evaluation of that formula, and a fifth of their windows were chosen unlike float64.  Against a float32 yardstick that
takes the cdf as 0.5 erfc (1e-6 to 1e-4 in those rows) that is two to four orders above the cap of 16.  `ct_cdf` is now 0.5 erfcf(-u / sqrt 2); the same rows read 1.1e-4 and below
(3 x 67, 12 positions in block 2) against a yardstick of 1.4e-4, and the choice cap holds over all channels.
REPORTED, not a failure: dW0 reads 9.05 x and dE 4.38 x the yardstick at 2 x 65,540, below the floor (dW0 7.3e-7 against 8.1e-8):
cnn_train_dt_kernel adds the 513 positions of a workgroup's chunk into its LDS table one after the other in fp32, the yardstick
sums a token's rows by torch's cascade.  At 2 x 16,421 (chunks of 129) the figure is below 1.
CHOICE: no window broke the gap rule, no exact float64 tie was decided another way, at most 5.2e-5 of a block's windows differed.
SCALING: dpooled x 2^-20 gave 2^-20 x every gradient and dz bit for bit at all five shapes, no element differing.
WRONG ON PURPOSE, two builds of csrc/cnn_train.hip under K = 8 (results only, every access inside its buffer; run on the parent's
GELU): ct_colsum never launching a last short workgroup fails test_rows at 5 x 2,053, 2 x 16,421 (both profiles) and 2 x 65,540 (and
tests/test_gpu_cnn_train.py, whose shapes have such a workgroup too); the dt kernel's second stretch keeping the first stretch's token
rows fails test_rows at 2 x 65,540 alone (dW0 1.5e-3, dE 2.2e-1 at token 0) and passes tests/test_gpu_cnn_train.py whole.
"""
from __future__ import annotations

import os

import pytest
import torch

import cnn_train_rows as R
import grad_rows as G

pytestmark = pytest.mark.gpu

K = R.K
K_CHOICE = 16 if K is None else K
SCALING_EXACT = True                                      # False: report only
SCALE, KEEP = 2.0 ** -20, 2.0 ** -60
CFG = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4], hidden_dim=512,
           number_of_classes=2, padding_idx=4)
_net = []


def _engine():
    """The training engine of one module, as tests/test_gpu_cnn_train.py test_backward_accumulates_with_beta_one drives it."""
    from chimeralm_amd.cnn import DNAConvNet

    if not _net:
        _net.append(DNAConvNet(**CFG, dropout=0.0, trainable=True))
    return _net[0].train_engine(torch.device("cuda", torch.cuda.current_device()))


def _run(inp, dp_scale: float = 1.0, fetch: bool = True) -> dict:
    """forward + backward on the engine -> the keys of `cnn_train_rows.evaluate` (CPU); the gradients land in NaN-filled buffers."""
    ids, params, keeps, scale, dpooled = inp
    eng = _engine()
    P = [p.cuda() for p in params]
    kp = None if keeps is None else [k.cuda() for k in keeps]
    pooled, mean, var, gen = eng.forward(ids.cuda(), P, kp, scale)
    grads = eng.backward(gen, (dpooled * dp_scale).cuda(), P, out=[torch.full_like(p, float("nan")) for p in P])
    torch.cuda.synchronize()
    got = {"pooled": pooled.cpu()}
    got.update({k: g.cpu() for k, g in zip(R.GRAD_KEYS, grads)})
    for i in range(3):
        got[f"mean{i}"], got[f"var{i}"] = mean[i].cpu(), var[i].cpu()
        got[f"dz{i}"] = torch.from_numpy(eng.debug_fetch(f"dz{i}"))
        if fetch:
            got[f"z{i}"], got[f"y{i}"] = torch.from_numpy(eng.debug_fetch(f"z{i}")), torch.from_numpy(eng.debug_fetch(f"y{i}"))
    if fetch:
        got["choice"] = [eng.debug_fetch(f"choice{i}") for i in range(3)]
    for k, v in got.items():
        if k != "choice":
            assert bool(torch.isfinite(v).all()), k
    return got


def _record(lines):
    print("\n".join(lines))
    if os.environ.get("CLM_CNN_TRAIN_ROWS"):
        with open(os.environ["CLM_CNN_TRAIN_ROWS"], "a") as f:
            f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_rows(built_lib, case):
    L, tag = case[2], R.case_id(case)
    inp = R.make_inputs(case)
    got = _run(inp)
    assert all(int(c.max()) < 4 for c in got["choice"])
    r64, r32 = R.evaluate(inp, torch.float64, choice=got["choice"]), R.evaluate(inp, torch.float32, choice=got["choice"])
    report = R.choice_report(got["choice"], r64, r32, K_CHOICE, L)
    _record(R.choice_lines(tag, report))
    eng_rows, yard_rows = R.rows(got, r64, L), R.rows(r32, r64, L)
    lines, bad, ratios = [], [], {}
    G.hold(tag, eng_rows, yard_rows, K, lines, bad, ratios)
    print("\n".join(lines))
    rms = lambda v: float(v.pow(2).mean().sqrt())                                    # noqa: E731
    _record([f"ROWS {tag:36s} {name:8s} engine max {G.worst(e):.2e} rms {rms(e):.2e}  yardstick max {G.worst(y):.2e} rms {rms(y):.2e}  "
             f"K {K}  worst ratio {ratios[name][0]:7.2f}  above the floor {ratios[name][1]:7.2f}"
             for (name, e, _), (_, y, _) in zip(eng_rows, yard_rows)])
    assert R.choice_ok(report), "\n".join(R.choice_lines(tag, report))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------- bit-exact relations
SAME = [R.SHAPES[2] + ("reads", "drop", "gamma"), R.SHAPES[2] + ("channels", "rows3", "offset"), R.SHAPES[5] + R.PLAIN]


@pytest.mark.parametrize("case", SAME, ids=R.case_id)
def test_second_call_is_identical(built_lib, case):
    inp = R.make_inputs(case)
    a, b = _run(inp, fetch=False), _run(inp, fetch=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", R.SHAPES[:4] + R.SHAPES[5:6], ids=lambda s: f"{s[1]}-{s[2]}-{s[3]}")
def test_scales_exactly(built_lib, shape):
    """dpooled x 2^-20: every step of the backward is linear in it (products with forward values, fp64 and MFMA sums, one rounding
    to fp32 each), so every gradient and dz scale by exactly 2^-20 while nothing is subnormal."""
    inp = R.make_inputs(shape + R.PLAIN)
    full, scaled = _run(inp, fetch=False), _run(inp, SCALE, fetch=False)
    assert torch.equal(full["pooled"], scaled["pooled"])
    ok = True
    for k in R.GRAD_KEYS + ["dz0", "dz1", "dz2"]:
        keep = full[k].abs() * SCALE >= KEEP
        same = (scaled[k] * (1.0 / SCALE) == full[k]) | ~keep
        _record([f"SCALING {shape[1]} x {shape[2]} {k}: {int(keep.sum())} of {keep.numel()} elements above 2^-60 after scaling, {int((~same).sum())} differ"])
        ok = ok and bool(same.all())
    if SCALING_EXACT:
        assert ok
