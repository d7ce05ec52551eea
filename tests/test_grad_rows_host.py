"""CPU: the yardstick, a second evaluation and planted defects of the row-wise gate of the training backward kernels
(tests/grad_rows.py; the engine's side is tests/test_gpu_grad_rows.py).

(a) CEILING.  For every case of the GPU file and every output, the float32 yardstick -- the hand formulas in float32, the kernel's
    algorithm: chunked for Mamba, FFT for Hyena -- stays below 1e-4 at EVERY row, so that K x yardstick is never a loose bound.
    Worst measured: 6.0e-5 (Mamba `steep`, dx), 2.4e-5 attention (`large`, dv), 3.3e-5 Hyena (dzc, 3 x 129 under the ramp).
(b) A SECOND float32 evaluation (torch autograd through the references' forwards; for Hyena also the dense `hand_core` up to
    L = 130) stays within 32 x the yardstick per read, max and rms over rows.  Mamba `steep` is printed only: there the chunked
    formulas lose digits that autograd through the same chunked forward loses elsewhere (exp(s_i - s_j) against exp(s_i) exp(-s_j)
    orderings), and neither is the other's bound.
(c) PLANTED DEFECTS, each in the float32 evaluation of the reference, never in the engine.  The row statistic must exceed
    max(16 x yardstick, 32 x 2^-24) at a row the defect reaches; the verdict of the existing tensor-wide gate
    (max |err| / max |fp64| <= max(8 x fp32, 32 x 2^-24)) is printed next to it.  Two items are not defects and are asserted as such:
    * Mamba `pad_dt` (rows t >= L of the last chunk staged with the dt of the rows behind them): dS is 0 in the last chunk and its
      exit state is never read, so exp(s_last) and exp(s_last - s_j) multiply zeros.  No output row moves.
    * Hyena's dk summed over the reads in float32: that IS the kernel (hyena_train_reduce_kernel adds the per-read rows in read
      order in float32) and the yardstick (`fft_core`'s .sum(0)).  Against a float64 sum it differs by at most B roundings of the
      channel's own denominator, 2^-22, below the floor; under `reads` the smaller read vanishes from dk in every arithmetic.
"""
from __future__ import annotations

import pytest
import torch

import attention_train_reference as AR
import grad_rows as G
import hyena_train_reference as HR
import mamba_train_reference as MR

# the ceiling, the second evaluation's factor, the planted defects' factor and the three comparisons live in tests/grad_rows.py
# (tests/test_cnn_train_rows_host.py shares them)
CEILING, K_SECOND, K_DEFECT = G.CEILING, G.K_SECOND, G.K_DEFECT
_ceiling, _argmax, _second, _planted = G.ceiling, G.argmax_row, G.second, G.planted


# ------------------------------------------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("pattern", AR.PATTERNS)
@pytest.mark.parametrize("case", G.ATTN_CASES, ids=G.case_id)
def test_attention_yardstick(case, pattern):
    (qkv, dout, keep), r64, r32 = G.attn_case(*case, pattern)
    tag = f"attention {G.case_id(case)} {pattern}"
    yard = G.attn_rows(r32, r64)
    _ceiling(tag, yard)
    _second(tag, G.attn_rows(AR.autograd(qkv, keep, case[2], dout), r64), yard)


@pytest.mark.parametrize("case", G.MAMBA_CASES, ids=G.case_id)
def test_mamba_yardstick(case):
    (zx, p, dout), r64, r32 = G.mamba_case(*case)
    tag = f"mamba {G.case_id(case)}"
    yard = G.mamba_rows(r32, r64)
    _ceiling(tag, yard)
    _second(tag, G.mamba_rows(MR.autograd_core(zx, p, dout), r64), yard, assert_it=case[5] != "steep")


@pytest.mark.parametrize("case", G.HYENA_CASES, ids=G.case_id)
def test_hyena_yardstick(case):
    inp, r64, r32 = G.hyena_case(*case)
    tag = f"hyena {G.case_id(case)}"
    yard = G.hyena_rows(r32, r64)
    _ceiling(tag, yard)
    _second(tag + " autograd", G.hyena_rows(HR.autograd_core(*inp), r64), yard)
    if case[1] <= 130:
        _second(tag + " dense", G.hyena_rows(HR.hand_core(*inp), r64), yard)


def test_profiles_are_powers_of_two():
    import grad_profiles as GP

    for name in GP.PROFILES:
        f = GP.factors(name, 3, 1031, 256)
        nz = f[f != 0]
        assert f.dtype == torch.float32 and bool((torch.frexp(nz)[0] == 0.5).all()), name
        assert float(nz.min()) >= 2.0 ** -GP.RAMP_CAP
    assert GP.support("rows3", 200).nonzero().flatten().tolist() == [0, 100, 199]
    assert GP.support("last_chunk", 200).nonzero().flatten().tolist() == list(range(192, 200))
    assert GP.support("first_chunk", 63).all() and int(GP.support("first_chunk", 200).sum()) == 64


# ------------------------------------------------------------------------------------------------------------- (c)
def _old_attention(ev, r64, r32):
    return [(k,) + G.old_gate(ev[k], r64[k], r32[k]) for k in ("out", "dq", "dk", "dv")]


def _old_mamba(ev, r64, r32):
    di, H, N = MR.dims_of({k: r64[k] for k in MR.CORE_PARAMS})
    d0 = 2 * di + 2 * N
    cut = lambda r, a, b: r["dzxbcdt"][..., a:b]                                     # noqa: E731
    out = [("out",) + G.old_gate(ev["out"], r64["out"], r32["out"]),
           ("dzxbcdt[z|xBC]",) + G.old_gate(cut(ev, 0, d0), cut(r64, 0, d0), cut(r32, 0, d0)),
           ("dzxbcdt[dt]",) + G.old_gate(cut(ev, d0, None), cut(r64, d0, None), cut(r32, d0, None), r64["dzxbcdt_dt_abs"])]
    for k in MR.CORE_PARAMS:
        out.append((f"d {k}",) + G.old_gate(ev[k], r64[k], r32[k], r64[k + "_abs"] if k in ("A_log", "dt_bias") else None))
    return out


def _old_hyena(ev, r64, r32):
    return [(k,) + G.old_gate(ev[k], r64[k], r32[k], r64["den"].get(k)) for k in ("c", "y") + HR.CORE_GRADS]


MAMBA_PLANTED = [  # (defect, case): what reaches which rows
    # the issue's own example, dout x 2^-(t // 8): what crosses a boundary backwards is 2^-8 of the rows it lands in.  The row gate
    # sees both in dx, dB and ddt; the tensor-wide gate sees the first by 1.2 x its bound in d conv1d.weight and is blind to the second
    ("carry_no_decay", (1, 128, 2, 200, "ramp_down", None)),
    ("carry_reset", (1, 128, 2, 200, "ramp_down", None)),
    ("conv_across_reads", (2, 64, 3, 65, "reads", None)),         # the last three rows of reads 0 and 1
    ("no_ub", (1, 128, 2, 200, "ramp_up", None)),                 # ddt of chunks 0 .. 2
]


@pytest.mark.parametrize("defect,case", MAMBA_PLANTED, ids=[d for d, _ in MAMBA_PLANTED])
def test_planted_mamba(defect, case):
    inp, r64, r32 = G.mamba_case(*case)
    ev = G.mamba_eval(inp, torch.float32, defect=defect)
    _planted(f"mamba {defect} at {G.case_id(case)}", G.mamba_rows(ev, r64), G.mamba_rows(r32, r64), _old_mamba(ev, r64, r32))


@pytest.mark.parametrize("profile", ["uniform", "ramp_up", "last_chunk"])
def test_mamba_pad_dt_reaches_no_row(profile):
    """Not a defect (module docstring): staging the dt of the rows behind a read into its ragged last chunk moves no output row."""
    case = (1, 128, 2, 200, profile, None)
    inp, r64, r32 = G.mamba_case(*case)
    ev = G.mamba_eval(inp, torch.float32, defect="pad_dt")
    _planted(f"mamba pad_dt at {G.case_id(case)}", G.mamba_rows(ev, r64), G.mamba_rows(r32, r64), _old_mamba(ev, r64, r32), expect_seen=False)


ATTN_PLANTED = [
    ("delta_unscaled", (2, 65, 0.1, "ramp_down"), "normal"),
    ("phantom_key", (3, 200, 0.0, "ramp_down"), "first_tile_max"),  # rows whose log-sum-exp is small feel the key of score 0
    ("skip_last_query_tile", (3, 200, 0.0, "rows3"), "normal"),     # position 199 carries a third of the gradient
]


@pytest.mark.parametrize("defect,case,pattern", ATTN_PLANTED, ids=[d for d, _, _ in ATTN_PLANTED])
def test_planted_attention(defect, case, pattern):
    inp, r64, r32 = G.attn_case(*case, pattern)
    ev = G.attn_eval(inp, torch.float32, defect=defect)
    _planted(f"attention {defect} at {G.case_id(case)} {pattern}", G.attn_rows(ev, r64), G.attn_rows(r32, r64), _old_attention(ev, r64, r32))


def _two_to_the_ten_apart():
    """v of the even channels x 2^10: the forward packs g of ch and ch + 1, the backward dc and g of one channel.  (The tensor-wide
    gate does not see c and y lose the odd channels' digits: it divides by the even channels' maximum.)"""
    zc, sw, sb, k, D, dy = G.hyena_inputs(2, 130, "uniform", "plain")
    zc = zc.clone()
    zc[:, 512::2] *= 2.0 ** 10
    return zc, sw, sb, k, D, dy


HYENA_PLANTED = [
    ("no_alias", lambda: G.hyena_inputs(3, 129, "ramp_down", "plain")),      # N = 256 = 2 L - 2
    ("unbalanced", _two_to_the_ten_apart),
    ("short_tail", lambda: G.hyena_inputs(2, 130, "ramp_up", "plain")),      # the tail carries the largest du
]


@pytest.mark.parametrize("defect,make", HYENA_PLANTED, ids=[d for d, _ in HYENA_PLANTED])
def test_planted_hyena(defect, make):
    inp = make()
    r64, r32 = G.hyena_eval(inp, torch.float64), G.hyena_eval(inp, torch.float32)
    n = 1 << HR.logn_for(inp[0].shape[-1])
    yard = G.hyena_rows(r32, r64)
    clean = HR.circular_mirror(*inp, n=n)                            # the kernels' form itself passes, so the variant is the defect
    _planted(f"hyena mirror form, no defect, B{inp[0].shape[0]} L{inp[0].shape[-1]}", G.hyena_rows(clean, r64), yard, _old_hyena(clean, r64, r32),
             expect_seen=False)
    ev = HR.circular_mirror(*inp, n=n, defect=defect)
    _planted(f"hyena {defect} B{inp[0].shape[0]} L{inp[0].shape[-1]}", G.hyena_rows(ev, r64), yard, _old_hyena(ev, r64, r32))


def test_hyena_dk_float32_read_sum_is_the_kernel():
    """Not a defect (module docstring): per-read dk rows from float32 transforms, summed over the reads in float32 (the kernel, the
    yardstick) and in float64, under `reads`.  Both sit at the yardstick; their difference is below the floor at every channel."""
    inp = G.hyena_inputs(3, 129, "reads", "plain")
    r64, r32 = G.hyena_eval(inp, torch.float64), G.hyena_eval(inp, torch.float32)
    per_read = [HR.fft_core(*(t[b:b + 1] if t.dim() == 3 else t for t in inp))["dk"] for b in range(3)]
    sum32, sum64 = per_read[0] + per_read[1] + per_read[2], sum(t.double() for t in per_read)
    den = r64["den"]["dk"].amax(-1)[None]
    s32, s64, y = (G._stat(t[None], r64["dk"][None], den) for t in (sum32, sum64, r32["dk"]))
    gap = G._stat(sum32[None], sum64[None], den)
    print(f"dk over reads: float32 sum {G.worst(s32):.3e}  float64 sum {G.worst(s64):.3e}  yardstick {G.worst(y):.3e}  "
          f"float32 against float64 sum {G.worst(gap):.3e}  floor {G.FLOOR:.3e}")
    assert G.worst(gap) <= 3 * 2.0 ** -24 and G.worst(s32) <= max(K_DEFECT * G.worst(y), G.FLOOR)
