"""The row-wise comparison of the training backward kernels (csrc/attention_train.hip, mamba_train.hip, hyena_train.hip) with float64:
the cases, the inputs, and for every output of an op its rows and their denominators.  Shared by tests/test_grad_rows_host.py (the
float32 yardstick, a second evaluation, planted defects; CPU) and tests/test_gpu_grad_rows.py (the engine).

The existing gate of these ops divides the largest error of a whole tensor by the largest entry of the whole tensor, and feeds the
backward a gradient of one size everywhere; it holds the largest rows only.  Here every output is cut into ROWS, each with its own
denominator, and `tf_stage_reference.statistic` / `check` hold every row (per read: the max and the rms over rows):

  attention   out                 per (position, head): the row's own max over the 32 components
              dq, dk, dv          per (position, head): max_d |err| over the row's sum of absolute terms (dS = p (dP - delta) cancels:
                                  the own-row maximum is not a denominator), attention_train_reference `dq_abs`, `dk_abs`, `dv_abs`
  mamba2      out, dz, dx, dB, dC per position, each column group on its own: the row's own max
              dt columns          per (position, head) over `dzxbcdt_dt_abs`
              d conv1d.weight, d conv1d.bias, d norm.weight per channel (and tap); dA_log, d dt_bias, dD per head: over `<key>_abs`
  hyena       c, y, dzc           per (read, channel) SEQUENCE: max_t |err| / max_t |ref| (a transform's error scales with the
                                  sequence, not with the sample)
              dk                  per channel: max_t |err| over max_t of the channel's sum of absolute terms
              dsw, dsb, dD        per channel likewise (`den` of hyena_train_reference)
  pooling     the head fine-tune's kernels (csrc/pool_train.hip): the table stands with its section below

A zero denominator demands an exact zero (statistic's rule).  A denominator below TINY = 2^-96 counts as TINY: fp32 holds 2^-24 of a
value only down to 2^-126, so a row of size d < 2^-96 whose ~2^10 terms each may lose 2^-126 (flushed or rounded as subnormals) cannot
be held to 2^-19 of d by any fp32 evaluation; it is held to that fraction of 2^-96 instead.
"""
from __future__ import annotations

from functools import lru_cache

import torch

import attention_train_reference as AR
import grad_profiles as GP
import headtrain_reference as HT
import hyena_train_reference as HR
import mamba_train_reference as MR
import tf_stage_reference as S

FLOOR = S.FLOOR
TINY = 2.0 ** -96
# engine <= max(K x yardstick, FLOOR), per op: measured on the MI355X, tests/test_gpu_grad_rows.py's docstring (None: measure only)
K = {"attention": 16, "mamba": 16, "hyena": 16, "pool": 16}     # (pool: tests/test_gpu_headtrain_rows.py's docstring)
SEED = 0x1234567887654321                      # the attention keep mask's
Q = 64                                         # Mamba's chunk, the attention's streamed tile
MAMBA_REGIMES = {"flat": ((1e-4, 1e-3), 1.0), "steep": ((1e-3, 2.0), 16.0)}     # tests/test_gpu_mamba_train.py REGIMES

# ------------------------------------------------------------------------------------------------------------- the cases
# attention (B, L, dropout p, profile), each under the five score patterns: a ragged second key tile | a ragged second 128-row owned
# tile, one read | three reads over ragged tiles | dropout | many tiles, several workgroups per (read, head)
ATTN_CASES = [(B, L, 0.0, prof) for (B, L) in ((2, 65), (1, 129), (3, 200)) for prof in ("uniform", "ramp_down", "rows3")]
ATTN_CASES += [(2, 65, 0.1, "uniform"), (2, 65, 0.1, "ramp_down"), (2, 1031, 0.0, "ramp_down")]
# Mamba2 core (expand, N, B, L, profile, regime): one short chunk | one token in the second chunk, H = 8 | dS carried over three
# boundaries at the register-critical N, a ragged last chunk of 8 | H = 12, a last chunk of 2
MAMBA_SHAPES = [(1, 16, 2, 63), (2, 64, 3, 65), (1, 128, 2, 200), (3, 32, 2, 130)]
MAMBA_PROFILES = ("uniform", "ramp_down", "ramp_up", "last_chunk", "first_chunk", "reads")
MAMBA_CASES = [s + (prof, None) for s in MAMBA_SHAPES for prof in MAMBA_PROFILES]
MAMBA_CASES += [(1, 128, 2, 200, prof, regime) for regime in sorted(MAMBA_REGIMES) for prof in ("ramp_up", "last_chunk")]
# Hyena core (B, L, profile, kind): logn 8 with the alias, odd B | logn 9 | logn 11 | logn 12 | logn 14 with the alias
HYENA_SHAPES = [(3, 129), (2, 130), (2, 700), (2, 1031)]
HYENA_PROFILES = ("uniform", "channels", "reads", "ramp_down", "rows3")
HYENA_CASES = [s + (prof, "plain") for s in HYENA_SHAPES for prof in HYENA_PROFILES]
HYENA_CASES += [(1, 8193, "channels", "plain"), (2, 700, "uniform", "disparate"), (2, 1031, "uniform", "decaying")]


def case_id(case) -> str:
    return "-".join(str(c) for c in case if c is not None)


# ------------------------------------------------------------------------------------------------------------- the inputs
def attn_inputs(B, L, p, profile, pattern):
    """(qkv, dout fp32, keep bool or None)."""
    dout = AR.make_dout(B, L) * GP.factors(profile, B, L, AR.D)
    keep = None if p == 0.0 else torch.from_numpy(AR.keep_mask(SEED, B, L, p))
    return AR.make_qkv(B, L, pattern), dout, keep


def mamba_inputs(expand, N, B, L, profile, regime):
    """(zxbcdt, params, dout) in fp32: the inputs of tests/test_gpu_mamba_train.py, dout shaped by the profile."""
    if regime is None:
        zx, p, dout = MR.random_core(100 + L, 256, expand, N, B, L, dtype=torch.float32)
    else:
        dt_range, A = MAMBA_REGIMES[regime]
        zx, p, dout = MR.random_core(7, 256, expand, N, B, L, dt_range=dt_range, A_value=A, dtype=torch.float32)
    return zx, p, dout * GP.factors(profile, B, L, expand * 256, Q)


def disparate(args):
    """tests/test_gpu_hyena_train.py test_core_op_disparate_scales: a training step's magnitudes."""
    zc, sw, sb, k, D, dy = args
    zc = zc.clone()
    zc[:, 512::2] *= 1e3                                             # v of the even channels
    return zc, sw, sb, k * 1e-3, D, dy * 1e-6


def hyena_inputs(B, L, profile, kind):
    """(zc, sw, sb, k, D, dy) in fp32.  `channels` and `reads` scale zc as well as dy (the forward packs channels ch, ch + 1; the
    reads must not see each other); the profiles along t scale dy alone."""
    if kind == "disparate":
        args = disparate(HR.random_core(11, B, L))
    elif kind == "decaying":
        args = HR.random_core(7, B, L, decaying_filter=True)
    else:
        args = HR.random_core(100 + L, B, L)
    zc, sw, sb, k, D, dy = args
    f = GP.factors(profile, B, L, HR.C).transpose(1, 2)              # broadcastable to [B, C, L]
    if profile in ("channels", "reads"):
        zc = zc * (f.repeat(1, 3, 1) if f.shape[1] > 1 else f)
    return zc, sw, sb, k, D, dy * f


# ------------------------------------------------------------------------------------------------------------- references
def attn_eval(inputs, dtype, defect=None):
    qkv, dout, keep = inputs
    p = 0.0 if keep is None else 0.1
    return AR.backward(qkv.to(dtype), keep, p, dout.to(dtype), defect=defect)


def mamba_eval(inputs, dtype, defect=None):
    zx, p, dout = inputs
    return MR.core_backward(zx.to(dtype), {k: v.to(dtype) for k, v in p.items()}, dout.to(dtype), defect=defect)


def hyena_eval(inputs, dtype):
    return HR.fft_core(*(t.to(dtype) for t in inputs))


@lru_cache(maxsize=2)
def attn_case(B, L, p, profile, pattern):
    """(inputs, float64 reference, float32 yardstick), computed once per case."""
    assert p in (0.0, 0.1)
    inp = attn_inputs(B, L, p, profile, pattern)
    return inp, attn_eval(inp, torch.float64), attn_eval(inp, torch.float32)


@lru_cache(maxsize=2)
def mamba_case(expand, N, B, L, profile, regime):
    inp = mamba_inputs(expand, N, B, L, profile, regime)
    return inp, mamba_eval(inp, torch.float64), mamba_eval(inp, torch.float32)


@lru_cache(maxsize=2)
def hyena_case(B, L, profile, kind):
    inp = hyena_inputs(B, L, profile, kind)
    return inp, hyena_eval(inp, torch.float64), hyena_eval(inp, torch.float32)


# ------------------------------------------------------------------------------------------------------------- rows
def _stat(got, ref, den=None):
    """statistic over rows [B, n, C] with the denominator [B, n] (default: the row's own maximum) raised to TINY where it is not 0."""
    ref = ref.double()
    den = ref.abs().amax(-1) if den is None else den.double()
    den = torch.where(den > 0, den.clamp_min(TINY), den)
    return S.statistic(got.detach().cpu().double(), ref, den)


def attn_rows(ev, r64):
    """[(output, statistic [B, L * 8], locate)] of an evaluation `ev` (keys out, dq, dk, dv: [B, L, 256]) against r64."""
    B, L, _ = r64["out"].shape
    cut = lambda t: t.reshape(B, L * AR.NH, AR.HD)                                   # noqa: E731  row = position * 8 + head

    def locate(b, i):
        t, h = divmod(i, AR.NH)
        return f"read {b} position {t} of {L} head {h}: 64-row tile {t // 64} (row {t % 64}), 128-row tile {t // 128}, last tile holds {(L - 1) % 64 + 1}"

    rows = [("out", _stat(cut(ev["out"]), cut(r64["out"])), locate)]
    for k in ("dq", "dk", "dv"):
        rows.append((k, _stat(cut(ev[k]), cut(r64[k]), r64[k + "_abs"].permute(0, 2, 1).reshape(B, L * AR.NH)), locate))
    return rows


def mamba_rows(ev, r64):
    """[(output, statistic, locate)] of `ev` (keys out, dzxbcdt and CORE_PARAMS) against r64 (`core_backward` in float64)."""
    di, H, N = MR.dims_of({k: r64[k] for k in MR.CORE_PARAMS})
    B, L, _ = r64["out"].shape

    def at(per):
        def locate(b, i):
            t = i // per
            return (f"read {b} position {t} of {L}" + (f" head {i % per}" if per > 1 else "") +
                    f": chunk {t // Q} of {(L + Q - 1) // Q}, row {t % Q} of {min(Q, L - t // Q * Q)} in it")
        return locate

    rows = [("out", _stat(ev["out"], r64["out"]), at(1))]
    o = 0
    for name, w in (("dz", di), ("dx", di), ("dB", N), ("dC", N)):
        rows.append((name, _stat(ev["dzxbcdt"][..., o:o + w], r64["dzxbcdt"][..., o:o + w]), at(1)))
        o += w
    flat = lambda t: t.reshape(B, L * H, 1)                                          # noqa: E731
    rows.append(("ddt", _stat(flat(ev["dzxbcdt"][..., o:]), flat(r64["dzxbcdt"][..., o:]), r64["dzxbcdt_dt_abs"].reshape(B, L * H)), at(H)))
    for k in MR.CORE_PARAMS:
        unit = "head" if r64[k].numel() == H else "channel"
        per = 4 if k == "conv1d.weight" else 1
        rows.append((f"d {k}", _stat(ev[k].reshape(1, -1, 1), r64[k].reshape(1, -1, 1), r64[k + "_abs"].reshape(1, -1)),
                     lambda b, i, unit=unit, per=per: f"{unit} {i // per}" + (f" tap {i % per}" if per > 1 else "")))
    return rows


def hyena_rows(ev, r64):
    """[(output, statistic, locate)] of `ev` (keys y, dzc, dsw, dsb, dk, dD and, where it has one, c) against r64 (`fft_core`)."""
    C = HR.C
    seq = lambda b, i: f"read {b} channel {i % C} (row {('x0', 'x1', 'v')[i // C]} of zc)" if i >= C else f"read {b} channel {i}"   # noqa: E731
    chan = lambda b, i: f"channel {i % C}" + (f" (row {('x0', 'x1', 'v')[i // C]})" if i >= C else "")   # noqa: E731
    rows = [(k, _stat(ev[k], r64[k]), seq) for k in ("c", "y", "dzc") if k in ev]
    rows.append(("dk", _stat(ev["dk"][None], r64["dk"][None], r64["den"]["dk"].amax(-1)[None]), chan))
    rows.append(("dsw", _stat(ev["dsw"][None], r64["dsw"][None], r64["den"]["dsw"].amax(-1)[None]), chan))
    for k in ("dsb", "dD"):
        rows.append((k, _stat(ev[k].reshape(1, -1, 1), r64[k].reshape(1, -1, 1), r64["den"][k].reshape(1, -1)), chan))
    return rows


# ------------------------------------------------------------------------------------------------------------- the head's pooling
# (csrc/pool_train.hip through Engine.pool_forward / pool_backward; tests/test_headtrain_rows_host.py and tests/test_gpu_headtrain_rows.py)
#
#   scores[b, t]   per token                  sum_f |w2_f g_f| + |b2|
#   attn[b, t]     per token                  its own value; the engine's from its scores and (max, sum) as pool_bwd_kernel takes it
#   pooled[b, c]   per (read, channel)        sum_t a_t |x_t,c|
#   dW1[f, c]      per element, reported per feature row f (the row's worst element)   sum_{b,t} |du_t,f| |x_t,c|
#   db1[f], dw2[f] per feature                sum |du_t,f|,  sum |ds_t g_t,f|
#   db2            the value against 0        sum |ds_t|
#
# Profiles, joined with "+", every scale an exact power of two:  plain (tests/test_gpu_headtrain.py's input) | b1_offsets: b1 +
# POOL_OFFSETS[f mod 8] | w2_ramp: w2_f x 2^-(f mod 13) | w1_rows: row f of W1 x 2^-(f mod 11) | dp_channels: dpooled[:, c] x 2^-(c mod 13)
# | peak<s>@<first|last|tile>: w2 x s (8: most of the softmax mass on one token, 40: almost all), and in every read the row with the
# highest fp64 score exchanged with the row at position 0, L - 1, or the first token of the last 64-token tile.
POOL_TILE, POOL_GRID, POOL_D = HT.TILE, 256, 256           # csrc/mfma32_common.h BM32, include/chimeralm_hip.h POOL_BWD_GRID
POOL_OFFSETS = (0.0, -3.0, -6.0, -8.0, 3.0, 6.0, -4.5, -5.5)
POOL_SEED = 1                                              # tests/test_gpu_headtrain.py's
POOL_FULL = ("plain", "b1_offsets", "w2_ramp", "w1_rows", "dp_channels", "peak8@first", "peak8@last", "peak8@tile", "peak40@first",
             "peak40@last", "peak40@tile", "b1_offsets+w2_ramp", "b1_offsets+peak8@last", "b1_offsets+peak40@last")
POOL_SHORT = ("plain", "b1_offsets", "peak8@last", "peak40@last")
# (B, L, profile): one token | one tile short of full, full, one token over | three tiles, the last of 2 | four tiles, the last of 8 |
# 257 one-tile reads on the 256-workgroup grid: workgroup 0 owns the tiles of reads 0 and 256 | 325 tiles, the one long case
POOL_CASES = [(B, L, q) for (B, L) in ((1, 65), (3, 200)) for q in POOL_FULL if not (q.endswith("@tile") and (L - 1) // POOL_TILE * POOL_TILE == L - 1)]
POOL_CASES += [(B, L, q) for (B, L) in ((1, 1), (1, 63), (3, 64), (2, 130), (257, 3)) for q in POOL_SHORT]
# dropped, both for the host file's 1e-4 ceiling on the float32 yardstick (ds_t = a_t ((x_t - p) . dp) cancels in itself where one token
# holds nearly all the mass, p is nearly x_t, and the denominators above take ds as given):
#   257 x 3 peak40@last breaks it (pooled of read 198, channel 12: 1.5e-4; that token's x_c is 1e-3 of its row, and ln_f rounds to 2^-24
#   of the row); 1 x 65 b1_offsets+peak40@last reads 7.2e-5 in dW1 on one CPU and 1.00e-4 on another (db1, dw2 alike: torch's float32
#   sums differ with the vector width).  It ran on the MI355X (engine 1.5e-4, ratio 1.49, profiles/headtrain_rows_parity.txt) and was
#   taken out because the host file would pass or fail by the machine.
POOL_CASES.remove((257, 3, "peak40@last"))
POOL_CASES.remove((1, 65, "b1_offsets+peak40@last"))
POOL_CASES += [(5, 4097, "plain"), (5, 4097, "b1_offsets+w2_ramp")]
POOL_GRADS = ("dW1", "db1", "dw2", "db2")


@lru_cache(maxsize=1)
def pool_sd():
    from oracle import hyena_oracle as ho

    return ho.make_state_dict(0)


def pool_inputs(B, L, profile):
    """`headtrain_reference.seeded_case` shaped by the profile: dict(rows, dpooled, lnf_g, lnf_b, w1, b1, w2, b2), fp32."""
    c = HT.seeded_case(B, L, seed=POOL_SEED, sd=pool_sd())
    f = torch.arange(POOL_D)
    for part in profile.split("+"):
        if part == "b1_offsets":
            c["b1"] = c["b1"] + torch.tensor(POOL_OFFSETS)[f % 8]
        elif part == "w2_ramp":
            c["w2"] = c["w2"] * torch.ldexp(torch.ones(POOL_D), -(f % 13))
        elif part == "w1_rows":
            c["w1"] = c["w1"] * torch.ldexp(torch.ones(POOL_D), -(f % 11))[:, None]
        elif part == "dp_channels":
            c["dpooled"] = c["dpooled"] * torch.ldexp(torch.ones(POOL_D), -(f % 13))
        elif part.startswith("peak"):
            scale, at = part[4:].split("@")
            c["w2"] = c["w2"] * float(scale)
            pos = {"first": 0, "last": L - 1, "tile": (L - 1) // POOL_TILE * POOL_TILE}[at]
            s = HT.pool_forward(c["rows"], c["lnf_g"], c["lnf_b"], c["w1"], c["b1"], c["w2"], c["b2"])["scores"]
            rows = c["rows"].clone()
            for b in range(B):
                top = int(s[b].argmax())
                rows[b, [top, pos]] = c["rows"][b, [pos, top]]
            c["rows"] = rows
        elif part != "plain":
            raise ValueError(profile)
    return {k: v.contiguous() for k, v in c.items()}


def pool_eval(c, dtype, defect=None, reverse=False):
    """forward + backward of the formulas in `dtype`: dict(scores, stats, attn, pooled, dW1, db1, dw2, db2, den)."""
    fwd, g = HT.pool_grads(c["rows"], c["lnf_g"], c["lnf_b"], c["w1"], c["b1"], c["w2"], c["b2"], c["dpooled"], dtype, defect, reverse)
    den = dict(fwd["den"], scores=fwd["scores_abs"], pooled=fwd["pooled_abs"])
    return {"scores": fwd["scores"], "stats": fwd["stats"], "attn": fwd["attn"], "pooled": fwd["pooled"], "den": den, **dict(zip(POOL_GRADS, g))}


@lru_cache(maxsize=2)
def pool_case(B, L, profile):
    """(inputs, float64 reference, float32 yardstick), computed once per case."""
    inp = pool_inputs(B, L, profile)
    return inp, pool_eval(inp, torch.float64), pool_eval(inp, torch.float32)


def pool_rows(ev, r64, grads=True):
    """[(output, statistic, locate)] of an evaluation `ev` (the keys of `pool_eval`; `attn` as given) against r64.  `grads` False: the
    forward's three outputs only (one token: every gradient is 0 and so is every denominator)."""
    B, L = r64["scores"].shape
    den, D = r64["den"], POOL_D
    tiles, last = (L + POOL_TILE - 1) // POOL_TILE, (L - 1) % POOL_TILE + 1
    tok = lambda b, t: (f"read {b} token {t} of {L}: 64-token tile {t // POOL_TILE} of {tiles} (global tile {b * tiles + t // POOL_TILE}, "   # noqa: E731
                        f"workgroup {(b * tiles + t // POOL_TILE) % POOL_GRID}), the last tile holds {last}")
    feat = lambda b, f: f"feature {f} (f mod 8 = {f % 8}, f mod 13 = {f % 13}, f mod 11 = {f % 11}); {B} x {tiles} tiles, the last holds {last}"   # noqa: E731
    chan = lambda b, i: f"read {b} channel {i} (c mod 13 = {i % 13}); {tiles} tiles, the last holds {last}"   # noqa: E731
    col = lambda t: t.reshape(t.shape[0], -1, 1)                                     # noqa: E731
    rows = [("scores", _stat(col(ev["scores"]), col(r64["scores"]), den["scores"]), tok),
            ("attn", _stat(col(ev["attn"]), col(r64["attn"])), tok),
            ("pooled", _stat(col(ev["pooled"]), col(r64["pooled"]), den["pooled"]), chan)]
    if grads:
        per = _stat(ev["dW1"].reshape(1, D * D, 1), r64["dW1"].reshape(1, D * D, 1), den["dW1"].reshape(1, D * D))
        rows.append(("dW1", per.reshape(1, D, D).amax(-1), feat))
        for k in ("db1", "dw2"):
            rows.append((k, _stat(ev[k].reshape(1, D, 1), r64[k].reshape(1, D, 1), den[k].reshape(1, D)), feat))
        rows.append(("db2", _stat(ev["db2"].reshape(1, 1, 1), torch.zeros(1, 1, 1, dtype=torch.float64), den["db2"].reshape(1, 1)),
                     lambda b, i: f"{B} x {tiles} tiles, the last holds {last}"))
    return rows


def pool_old_gates(ev, r64, r32):
    """[(output, error, bound)] of the tensor-wide gate of tests/test_gpu_headtrain.py (db2 against dw2's bound and scale, as there)."""
    res = [(k,) + old_gate(ev[k], r64[k], r32[k]) for k in ("pooled", "dW1", "db1", "dw2")]
    scale = float(r64["dw2"].abs().max())
    return res + [("db2", abs(float(ev["db2"])) / scale if scale > 0 else abs(float(ev["db2"])), res[-1][2])]


# ------------------------------------------------------------------------------------------------------------- the comparison
def hold(tag, eng_rows, yard_rows, K, lines, bad, ratios=None):
    """`check` of every output: engine <= max(K x yardstick, FLOOR) per read for the max and the rms over rows (K None: measures).
    The lines name the worst row through the output's `locate`.  `ratios`: {output: [worst ratio, worst above the floor]}, updated."""
    for (name, e, loc), (_, y, _) in zip(eng_rows, yard_rows):
        n0, b0 = len(lines), len(bad)
        worst, above = S.check(tag, name, e, y, K, lines, bad)
        where = [loc(b, int(e[b].argmax())) for b in range(e.shape[0]) for _ in (0, 1)]
        failed = set(bad[b0:])
        for i, w in enumerate(where):
            fixed = lines[n0 + i].split("  worst: ")[0] + "  worst: " + w
            if lines[n0 + i] in failed:
                bad[bad.index(lines[n0 + i], b0)] = fixed
            lines[n0 + i] = fixed
        if ratios is not None:
            r = ratios.setdefault(name, [0.0, 0.0])
            r[0], r[1] = max(r[0], worst), max(r[1], above)


def old_gate(got, r64, r32, den=None) -> tuple[float, float]:
    """The tensor-wide gate of the existing tests: (max |got - fp64| / max |den|, its bound max(8 x the same of fp32, FLOOR))."""
    d = float((r64 if den is None else den).double().abs().max().clamp_min(1e-300))
    err = float((got.double() - r64).abs().max()) / d
    return err, max(8.0 * float((r32.double() - r64).abs().max()) / d, FLOOR)


def worst(stat: torch.Tensor) -> float:
    return float(stat.max())


def summary(ratios: dict) -> list[str]:
    return [f"RATIO {k:18s} worst engine / yardstick {v[0]:8.2f}   above the floor {v[1]:8.2f}" for k, v in ratios.items()]


# ------------------------------------------------------------------------------------------------------------- the host files' comparisons
# (tests/test_grad_rows_host.py and tests/test_cnn_train_rows_host.py: the yardstick's ceiling, a second evaluation, planted defects)
CEILING = 1e-4
K_SECOND = 32
K_DEFECT = 16


def ceiling(tag, rows):
    lines = [f"CEILING {tag:44s} {name:16s} yardstick max {worst(st):.3e}  worst: {loc(*argmax_row(st))}" for name, st, loc in rows]
    print("\n".join(lines))
    bad = [ln for ln, (_, st, _) in zip(lines, rows) if not worst(st) < CEILING]
    assert not bad, "\n".join(bad)


def argmax_row(st):
    b = int(st.amax(1).argmax())
    return b, int(st[b].argmax())


def second(tag, second_rows, yard_rows, assert_it=True):
    names = {n for n, _, _ in second_rows}
    lines, bad = [], []
    hold(tag, second_rows, [r for r in yard_rows if r[0] in names], K_SECOND, lines, bad)
    print("\n".join(lines))
    if assert_it:
        assert not bad, "\n".join(bad)
    elif bad:
        print("(reported only)\n" + "\n".join(bad))



def planted(tag, defect_rows, yard_rows, old, expect_seen=True):
    """The row gate's verdict on a planted variant (asserted) and the tensor-wide gate's (printed)."""
    seen = []
    for (name, d, loc), (_, y, _) in zip(defect_rows, yard_rows):
        over = d / torch.clamp(K_DEFECT * y, min=FLOOR)
        if float(over.max()) > 1.0:
            b, i = argmax_row(over)
            seen.append(f"{name}: {float(d[b, i]):.3e} against max(16 x {float(y[b, i]):.3e}, floor) at {loc(b, i)}; "
                        f"{int((over > 1).sum())} of {over.numel()} rows")
    old_seen = [f"{n} {e:.3e} > {bnd:.3e}" for n, e, bnd in old if not e <= bnd]
    print(f"PLANTED {tag}\n  row gate:         " + ("SEES " + "\n                    ".join(seen) if seen else "blind") +
          "\n  tensor-wide gate: " + ("SEES " + "; ".join(old_seen) if old_seen else "blind (worst " +
                                      max((f"{e / bnd:.3f} of its bound, {n}" for n, e, bnd in old), key=lambda s: float(s.split()[0])) + ")"))
    assert bool(seen) == expect_seen, tag
    return bool(old_seen)
