"""GPU (MI355X): the training kernels of the three cores -- csrc/attention_train.hip, mamba_train.hip, hyena_train.hip -- against
float64 ROW BY ROW, under gradients shaped like a training step's.

tests/test_gpu_attention_train.py, test_gpu_mamba_train.py and test_gpu_hyena_train.py divide the largest error of a whole tensor by
the largest entry of the whole tensor and feed the backward a unit-normal gradient: they hold the largest rows.  Here every output is
cut into rows with a denominator of their own (tests/grad_rows.py: per (position, head) over the sum of absolute terms for the
attention; per position and column group for the Mamba2 core; per (read, channel) sequence for the Hyena core; per channel or head for
the batch-reduced gradients), the gradient follows tests/grad_profiles.py (uniform, ramps of 2^-(t // 8), three rows, one chunk,
per-channel and per-read scales), and the bound is, per read, for the max and the rms over rows,

    engine <= max(K x yardstick, 32 x 2^-24)        yardstick: the same formulas in float32 on the CPU, never the engine.

tests/test_grad_rows_host.py holds that yardstick below 1e-4 at every row of every case here and shows what the gate does with
planted defects.  A zero denominator demands an exact zero: in `rows3` the dq rows of positions without dout, under `first_chunk` every
row of dz, dx, dB, dC and ddt behind the chunk and the conv's three tokens (asserted on their own as well).

BIT-EXACT RELATIONS, asserted as such: a second call gives identical bits under every non-uniform profile (one shape per op); scaling
dout by 2^-20 scales every gradient of the attention and the Mamba2 core by exactly 2^-20 wherever the scaled gradient stays above
2^-60 (below, a term may be subnormal).  For the Hyena core the same relation is SCALING_EXACT_HYENA (see below).

K, from the first run (no bound set before it; CLM_GRAD_ROWS_PARITY=<file> appends every line; profiles/grad_rows_parity.txt is that
run): per op the worst engine / yardstick ratio among figures above the floor, over cases, reads and both statistics; K = the smallest
power of two >= 2 x that ratio, capped at 16.
    attention  4.56  (out, 2 x 1031 ramp_down, `flat`: 1.93e-6 against 4.24e-7, max over rows) -> 2 x 4.56 = 9.1  -> K = 16
    mamba2     6.83  (d conv1d.weight, 1 x N128 x B2 x L200 ramp_up, `steep`)                -> 2 x 6.83 = 13.7 -> K = 16
    hyena      6.59  (dzc, 3 x 129 ramp_down)                                                -> 2 x 6.59 = 13.2 -> K = 16
No figure exceeds the cap of 16 and no kernel was changed.  Outside `steep` the Mamba2 core stays at or below 3.5 x.

MEASURED on the MI355X, this tree, K unset: the worst engine / yardstick ratio over cases, reads and both statistics (all figures |
those above the floor of 1.9e-6), and the largest row statistic of the engine and of the yardstick over all cases.  133 tests in 10 s.
    op         output           all    above  engine max  yardstick max
    attention  out               4.56   4.56  1.62e-05    1.88e-05
    attention  dq                3.64   1.39  3.97e-06    2.86e-06
    attention  dk                2.00   2.00  1.25e-05    8.71e-06
    attention  dv                1.98   1.64  2.24e-05    2.43e-05
    mamba      out               2.47   2.17  5.41e-05    2.57e-05
    mamba      dz                2.85   1.79  2.40e-05    3.13e-05
    mamba      dx                3.52   3.52  1.03e-04    6.01e-05
    mamba      dB                5.12   5.12  1.62e-04    5.73e-05
    mamba      dC                5.34   5.34  1.56e-04    5.07e-05
    mamba      ddt               5.46   5.46  9.46e-05    1.73e-05
    mamba      d conv1d.weight   6.83   6.83  2.98e-05    6.16e-06
    mamba      d conv1d.bias     6.27   6.27  1.10e-05    1.90e-06
    mamba      d dt_bias         3.39  -      2.19e-08    2.76e-08
    mamba      d A_log           4.32  -      1.47e-08    2.18e-08
    mamba      d D               2.28  -      1.71e-07    9.62e-08
    mamba      d norm.weight     3.97   3.97  9.73e-06    2.60e-06
    hyena      c                 3.08   1.40  1.99e-06    1.91e-06
    hyena      y                 2.86   1.14  2.19e-06    2.21e-06
    hyena      dzc               6.59   6.59  8.08e-05    4.47e-05
    hyena      dk                5.74   3.43  2.94e-06    8.58e-07
    hyena      dsw               2.76   2.76  5.71e-06    4.87e-06
    hyena      dsb               7.67   4.89  6.24e-06    3.63e-06
    hyena      dD                1.47  -      3.51e-07    6.18e-07
("-": no figure of that output reached the floor.)
SCALING: dout x 2^-20 gave 2^-20 x every gradient bit for bit, no element differing, in all 15 attention cases (`large` included) and
all 4 Mamba2 shapes.  The Hyena core does NOT scale bit for bit (a quarter of dzc, half of dk differ in the last place; dD, which takes
no transform, is exact): hyena_train_balance halves the difference of the two exponents with a truncating division, so dy x 2^-20
moves the balancing power of an odd difference by 2^-19 or 2^-21 and the packed signal rounds elsewhere.  Reported, not asserted
(SCALING_EXACT_HYENA); both results sit inside the bound above.
"""
from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

import attention_train_reference as AR
import grad_profiles as GP
import grad_rows as G
import hyena_train_reference as HR
import mamba_train_reference as MR

pytestmark = pytest.mark.gpu

K = G.K                                                   # x the float32 yardstick, per op (the module docstring has the measurement)
SCALING_EXACT_HYENA = False                               # False: report only
TAIL = 16                                                 # floats (64 bytes) of sentinel behind every attention output
SCALE = 2.0 ** -20
KEEP = 2.0 ** -60


# ------------------------------------------------------------------------------------------------------------- the ops
def _lib():
    from chimeralm_amd import _native as N

    return N.load()


def _buf(n: int) -> torch.Tensor:
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")


def _take(buf: torch.Tensor, shape, what: str) -> torch.Tensor:
    n = 1
    for s in shape:
        n *= s
    assert torch.isnan(buf[n:]).all(), f"{what}: bytes past its end were written"
    return buf[:n].reshape(shape)


def _attention(qkv_cpu, dout_cpu, p):
    """clm_attn_train_forward + clm_attn_train_backward through ctypes, NaN sentinels behind every buffer -> out, dq, dk, dv (CPU)."""
    lib, st = _lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qkv, dout = qkv_cpu.cuda(), dout_cpu.cuda()
    B, L, _ = qkv.shape
    out, lse, dqkv = _buf(B * L * 256), _buf(B * 8 * L), _buf(B * L * 768)
    assert lib.clm_attn_train_forward(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, p, G.SEED, st) == 0
    n = int(lib.clm_attn_train_workspace_bytes(B, L))
    ws = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.clm_attn_train_backward(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
                                       B, L, p, G.SEED, st) == 0
    torch.cuda.synchronize()
    assert bool((ws[n:] == 0x5A).all()), "workspace: bytes past its end were written"
    _take(lse, (B, 8, L), "lse")
    d = _take(dqkv, (B, L, 768), "dqkv").cpu()
    return {"out": _take(out, (B, L, 256), "out").cpu(), "dq": d[..., :256], "dk": d[..., 256:512], "dv": d[..., 512:]}


def _mamba(zx, p, dout, dims):
    """Mamba2Core.apply and its backward -> the outputs under the reference's names (CPU)."""
    from chimeralm_amd.mambatrain import Mamba2Core, MambaTrainEngine

    eng = MambaTrainEngine(torch.device("cuda", torch.cuda.current_device()))
    zg = zx.cuda().requires_grad_(True)
    pg = [p[k].cuda().requires_grad_(True) for k in MR.CORE_PARAMS]
    out = Mamba2Core.apply(eng, dims, zg, *pg)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dzxbcdt": zg.grad.cpu()}
    res.update({k: t.grad.cpu() for k, t in zip(MR.CORE_PARAMS, pg)})
    eng.close()
    return res


def _hyena(args):
    """hyenatrain.core_forward + core_backward -> c, y and the five gradients (CPU)."""
    from chimeralm_amd import hyenatrain as ht

    zc, sw, sb, k, D, dy = (t.contiguous().cuda() for t in args)
    c, y = ht.core_forward(zc, sw, sb, k, D)
    grads = ht.core_backward(zc, sw, sb, k, D, c, dy)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in zip(("c", "y") + HR.CORE_GRADS, (c, y) + tuple(grads))}


# ------------------------------------------------------------------------------------------------------------- the comparison
def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_GRAD_ROWS_PARITY"):
        with open(os.environ["CLM_GRAD_ROWS_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _hold(op, tag, got, eng_rows, yard_rows):
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (tag, k)
    lines, bad, ratios = [], [], {}
    G.hold(tag, eng_rows, yard_rows, K[op], lines, bad, ratios)
    print("\n".join(lines))
    rms = lambda v: float(v.pow(2).mean().sqrt())                                    # noqa: E731
    _record([f"ROWS {op:9s} {tag:44s} {name:16s} engine max {G.worst(e):.2e} rms {rms(e):.2e}  yardstick max {G.worst(y):.2e} rms {rms(y):.2e}  "
             f"K {K[op]}  worst ratio {ratios[name][0]:7.2f}  above the floor {ratios[name][1]:7.2f}"
             for (name, e, _), (_, y, _) in zip(eng_rows, yard_rows)])
    assert not bad, "\n".join(bad)


def _scales_exactly(tag, full: dict, scaled: dict) -> bool:
    """scaled == full x 2^-20 bit for bit wherever |full| x 2^-20 >= 2^-60.  Prints the share of the elements that takes part."""
    ok = True
    for k in full:
        keep = full[k].abs() * SCALE >= KEEP
        same = (scaled[k] * (1.0 / SCALE) == full[k]) | ~keep
        print(f"SCALING {tag} {k}: {int(keep.sum())} of {keep.numel()} elements above 2^-60 after scaling, {int((~same).sum())} differ")
        ok = ok and bool(same.all())
    return ok


# ------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("pattern", AR.PATTERNS)
@pytest.mark.parametrize("case", G.ATTN_CASES, ids=G.case_id)
def test_attention_rows(built_lib, case, pattern):
    B, L, p, profile = case
    (qkv, dout, keep), r64, r32 = G.attn_case(*case, pattern)
    got = _attention(qkv, dout, p)
    if profile == "rows3":                                             # (also the zero-denominator rule of the statistic)
        off = ~GP.support("rows3", L)
        assert float(got["dq"][:, off].abs().max()) == 0.0, "dq of a position without dout is not exactly 0"
    _hold("attention", f"{G.case_id(case)} {pattern}", got, G.attn_rows(got, r64), G.attn_rows(r32, r64))


@pytest.mark.parametrize("profile", ["ramp_down", "rows3"])
def test_attention_second_call_is_identical(built_lib, profile):
    for pattern in AR.PATTERNS:
        qkv, dout, _ = G.attn_inputs(3, 200, 0.1, profile, pattern)
        a, b = _attention(qkv, dout, 0.1), _attention(qkv, dout, 0.1)
        for k in a:
            assert torch.equal(a[k], b[k]), (pattern, k)


@pytest.mark.parametrize("B,L", [(2, 65), (1, 129), (3, 200)])
def test_attention_scales_exactly(built_lib, B, L):
    """`large` is printed only: its probabilities reach fp32's subnormals whatever dout is, and their products with dout x 2^-20
    round there."""
    for pattern in AR.PATTERNS:
        qkv, dout, _ = G.attn_inputs(B, L, 0.0, "uniform", pattern)
        full, scaled = _attention(qkv, dout, 0.0), _attention(qkv, dout * SCALE, 0.0)
        grads = lambda r: {k: r[k] for k in ("dq", "dk", "dv")}                     # noqa: E731
        assert torch.equal(full["out"], scaled["out"])
        ok = _scales_exactly(f"attention B{B} L{L} {pattern}", grads(full), grads(scaled))
        assert ok or pattern == "large", pattern


# ------------------------------------------------------------------------------------------------------------- Mamba2 core
@pytest.mark.parametrize("case", G.MAMBA_CASES, ids=G.case_id)
def test_mamba_rows(built_lib, case):
    expand, N, B, L, profile, regime = case
    (zx, p, dout), r64, r32 = G.mamba_case(*case)
    got = _mamba(zx, p, dout, (256, expand, N))
    if profile == "first_chunk" and L > G.Q + 3:                       # behind the chunk and the conv's three-token reach
        assert float(got["dzxbcdt"][:, G.Q + 3:].abs().max()) == 0.0, "a row behind the first chunk is not exactly 0"
    _hold("mamba", G.case_id(case), got, G.mamba_rows(got, r64), G.mamba_rows(r32, r64))


@pytest.mark.parametrize("profile", [q for q in G.MAMBA_PROFILES if q != "uniform"])
def test_mamba_second_call_is_identical(built_lib, profile):
    zx, p, dout = G.mamba_inputs(1, 128, 2, 200, profile, None)
    a, b = _mamba(zx, p, dout, (256, 1, 128)), _mamba(zx, p, dout, (256, 1, 128))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", G.MAMBA_SHAPES, ids=G.case_id)
def test_mamba_scales_exactly(built_lib, shape):
    expand, N, B, L = shape
    zx, p, dout = G.mamba_inputs(expand, N, B, L, "uniform", None)
    full, scaled = _mamba(zx, p, dout, (256, expand, N)), _mamba(zx, p, dout * SCALE, (256, expand, N))
    assert torch.equal(full.pop("out"), scaled.pop("out"))
    assert _scales_exactly(f"mamba {G.case_id(shape)}", full, scaled)


# ------------------------------------------------------------------------------------------------------------- Hyena core
@pytest.mark.parametrize("case", G.HYENA_CASES, ids=G.case_id)
def test_hyena_rows(built_lib, case):
    inp, r64, r32 = G.hyena_case(*case)
    got = _hyena(inp)
    _hold("hyena", G.case_id(case), got, G.hyena_rows(got, r64), G.hyena_rows(r32, r64))


@pytest.mark.parametrize("profile", [q for q in G.HYENA_PROFILES if q != "uniform"])
def test_hyena_second_call_is_identical(built_lib, profile):
    inp = G.hyena_inputs(3, 129, profile, "plain")
    a, b = _hyena(inp), _hyena(inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("B,L", G.HYENA_SHAPES)
def test_hyena_scaling(built_lib, B, L):
    """dy x 2^-20: the backward packs dc + i g, balanced by a power of two taken from the two sums of squares
    (hyena_train_balance); the power follows dy's scale, so the packed signal is the same and the gradients scale exactly -- if the
    balancing step's truncating division lands on the same side.  SCALING_EXACT_HYENA says what the first run showed."""
    zc, sw, sb, k, D, dy = G.hyena_inputs(B, L, "uniform", "plain")
    full, scaled = _hyena((zc, sw, sb, k, D, dy)), _hyena((zc, sw, sb, k, D, dy * SCALE))
    for name in ("c", "y"):
        assert torch.equal(full.pop(name), scaled.pop(name)), name
    ok = _scales_exactly(f"hyena B{B} L{L}", full, scaled)
    _record([f"SCALING hyena B{B} L{L}: every gradient of dy x 2^-20 is 2^-20 x the gradient, bit for bit: {ok}"])
    if SCALING_EXACT_HYENA:
        assert ok
