"""The row-wise comparison of DNAConvNet's training kernels (csrc/cnn_train.hip) with float64: the cases, the inputs, the op restated
explicitly in torch, and for every output its rows and their denominators.  Shared by tests/test_cnn_train_rows_host.py (the float32
yardstick, a second evaluation, planted defects; CPU) and tests/test_gpu_cnn_train_rows.py (the engine).  Modelled on tests/grad_rows.py,
whose `hold`, `old_gate`, `_stat` (tf_stage_reference's `statistic` and `check` under them), FLOOR and TINY it uses.

THE OP is `CnnTrainEngine.forward(ids, params, keeps, scale)` followed by `backward(gen, dpooled, params)`: cut at `pooled`, `dpooled`
an input, no fc head, no loss, routed by a given pooling `choice`.  `evaluate` writes every formula out (tests/cnn_train_reference.py
leaves the backward to autograd; tests/test_cnn_train_rows_host.py pins this file's backward to that autograd in float64), because
every cancelling sum also returns the sum of the absolute values of its terms, one level deep (the inputs of a sum taken as given):

  output                       row                          denominator
  z_i, y_i, pooled             per position / per read      the row's own maximum over the 256 channels
  batch mean_i                 per channel                  sum |z| / n
  batch var_i                  per channel                  its own value
  dz_i                         per position                 |g| rstd (|dy| + |m1| + |xh m2|), the maximum over the row's channels; for i < 2
                                                            |dy| = |gelu'| x keep scale x conv(|dz_{i+1}|, |W_{i+1}|) at the chosen position
  dW_i                         per (co, tap), 256 ci wide   sum_{b, t} |dz| |x|, the maximum over ci
  dg_i, dbeta_i, db_i          per channel                  sum |dy xh|, sum |dy|, sum |dz| (db_i is 0 in exact arithmetic)
  d embedding                  per token row                sum |dT| |W_0|, the maximum over ci; 0 for row 4 (padding_idx)

A zero denominator demands an exact zero (a token absent from the batch, row 4); a denominator below TINY counts as TINY.

INPUT PROFILES, every factor an exact power of two:
  dpooled   uniform: seeded unit normal | channels: x 2^-(c mod 13) | reads: x 2^-(10 b)
  keeps     none | drop: Bernoulli 0.9, scale fp32(1 / 0.9) | rows3: block 2's mask 1 at pooled positions 0, L_3 // 2, L_3 - 1 only
            (at L = 203, L_3 = 3 and the mask is all ones: the profile bites from 2 x 1,031, L_3 = 16, on)
  params    plain | gamma: BatchNorm weights x 2^-(c mod 13) | convrows: W_i[co], b_i[co] x 2^-(co mod 11) (the smallest channels'
            variance is below eps) | offset: b_i + 64 on every fourth channel | dead: BatchNorm bias -6 on the odd channels
  ids       cnn_reference.synthetic_ids, token 0 exactly once (position 0 of read 0), token 1 exactly once (the last position of the
            last read: its windows reach outside the read)

THE POOLING CHOICE is compared with the engine's own (a near-tie decided the other way in fp32 is not an error) and held by
`choice_report`: the chosen element may differ from float64's first maximum only where the float64 gap between the two is at most
max(K x the channel's largest |y32 - y64| of the float32 yardstick, FLOOR x the channel's max |y64|), an exact float64 tie is decided as
torch decides it, and at most 0.05 % of a block's windows differ, over all channels and under every profile.

SEEDS: one per shape.  Block 2 of 2 x 64 has 8 positions and of 3 x 67 has 12, a channel's variance over so few can be small, and under
`offset` (z = 64 + ..., held to 2^-24 of 64) the float32 dW_2 rows then sit at 1e-4 to 2e-4 for most seeds; 29 and 5 are seeds at
which the yardstick stays below the ceiling of tests/test_cnn_train_rows_host.py for every profile.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

import cnn_reference as cr
import grad_profiles as GP
import grad_rows as G

FLOOR, TINY = G.FLOOR, G.TINY
C, KW, HALO, VOC, EPS, PAD = 256, 7, 3, 12, 1e-5, 4
K = 8                                          # engine <= max(K x yardstick, FLOOR): tests/test_gpu_cnn_train_rows.py's docstring (None: measure only)
DIFFER_CAP = 5e-4                              # of a block's windows, tests/test_gpu_cnn_train.py's
DROP_SCALE = float(np.float32(1.0 / 0.9))
# csrc/cnn_train.hip: CT_STAT_GRID (stats, dy), CT_DT_GRID, CT_DW_GRID, CT_DT_SUB, and the minimum chunks of the three ct_split calls
STAT_GRID, DT_GRID, DW_GRID, DT_SUB, SLICES = 512, 256, 36, 512, 4
STAT_MIN, DY_MIN, DT_MIN = 64, 16, 128

# ------------------------------------------------------------------------------------------------------------- the cases
# (seed, B, L, pads): one tile everywhere, L_3 = 1 | positions past 4 L_out in block 0 | L_1 = 50, L_2 = 12: uncovered positions in
# block 1, exact ties in the pad prefix | L_1 = 257 (a last tile of one row), L_2 = 64 | 45 block-1 tiles on the 36-workgroup dw grid |
# n = 32,842: every chunked kernel above its minimum chunk, grids below the cap | n = 131,080: the dt kernel's second staging stretch
SHAPES = [(29, 2, 64, 0), (5, 3, 67, 0), (2, 3, 203, 17), (3, 2, 1031, 100), (4, 5, 2053, 0), (5, 2, 16421, 0), (6, 2, 65540, 0)]
PLAIN = ("uniform", "none", "plain")
PROFILES = [PLAIN, ("channels", "none", "plain"), ("reads", "none", "plain"), ("uniform", "drop", "plain"), ("uniform", "rows3", "plain"),
            ("uniform", "none", "gamma"), ("uniform", "none", "convrows"), ("uniform", "none", "offset"), ("uniform", "none", "dead")]
CROSSED = [("reads", "drop", "gamma"), ("channels", "drop", "convrows"), ("channels", "none", "gamma")]
CASES = [s + p for s in SHAPES[:3] for p in PROFILES if p[1] != "rows3" or s[2] >= 192]
CASES += [s + p for s in SHAPES[1:3] for p in CROSSED]     # (not at 2 x 64: over block 2's 8 positions a crossed yardstick passes 1e-4)
CASES += [s + PLAIN for s in SHAPES[3:]] + [SHAPES[5] + ("reads", "none", "plain")]
CASES += [SHAPES[3] + ("uniform", "rows3", "plain"), SHAPES[4] + ("channels", "rows3", "plain")]      # L_3 = 16 and 32: 3 kept positions


def case_id(case) -> str:
    return "-".join(str(c) for c in case[1:])


def lens(L: int) -> list[int]:
    return [L, L // 4, L // 16, L // 64]


def ct_split(n: int, max_grid: int, min_chunk: int) -> tuple[int, int]:
    """csrc/cnn_train.hip ct_split: (chunk, grid)."""
    g = max(1, min(-(-n // min_chunk), max_grid))
    chunk = -(-n // g)
    return chunk, -(-n // chunk)


def slices(parts: int) -> list[int]:
    """How many of `parts` partials each of the four slices of stats_final / dt_reduce adds."""
    per = -(-parts // SLICES)
    return [max(0, min(parts, (s + 1) * per) - s * per) for s in range(SLICES)]


# ------------------------------------------------------------------------------------------------------------- the inputs
@lru_cache(maxsize=8)
def _state_dict(seed: int) -> dict:
    return cr.make_cnn_state_dict(seed)


def make_ids(seed: int, B: int, L: int, pads: int) -> torch.Tensor:
    ids = cr.synthetic_ids(seed, B, L, pads)
    ids[ids < 2] = 2                           # tokens 0 and 1 are placed, not drawn
    ids[0, 0] = 0
    ids[B - 1, L - 1] = 1
    return torch.from_numpy(ids)


def make_params(seed: int, profile: str) -> list[torch.Tensor]:
    """The 13 engine parameters (embedding, then W, b, g, beta per block) in fp32, shaped by the profile."""
    sd = _state_dict(seed)
    ps = [sd["embedding.weight"].clone()]
    c = torch.arange(C)
    for i in range(3):
        W, b, g, beta = (sd[f"conv_blocks.{i}.{k}"].clone() for k in ("0.weight", "0.bias", "1.weight", "1.bias"))
        if profile == "gamma":
            g = g * torch.ldexp(torch.ones(C), -(c % 13))
        elif profile == "convrows":
            f = torch.ldexp(torch.ones(C), -(c % 11))
            W, b = W * f[:, None, None], b * f
        elif profile == "offset":
            b[::4] += 64.0
        elif profile == "dead":
            beta[1::2] = -6.0
        elif profile != "plain":
            raise ValueError(profile)
        ps += [W, b, g, beta]
    return [p.float().contiguous() for p in ps]


def make_keeps(seed: int, B: int, L: int, profile: str):
    """(three uint8 masks [B, L_{i+1}, 256] or None, scale)."""
    Ls = lens(L)
    if profile == "none":
        return None, 1.0
    if profile == "drop":
        gen = torch.Generator().manual_seed(77 + seed)
        return [(torch.rand((B, Ls[i + 1], C), generator=gen) < 0.9).to(torch.uint8) for i in range(3)], DROP_SCALE
    if profile == "rows3":
        assert Ls[3] >= 3
        keeps = [torch.ones((B, Ls[i + 1], C), dtype=torch.uint8) for i in range(3)]
        keeps[2].zero_()
        keeps[2][:, [0, Ls[3] // 2, Ls[3] - 1]] = 1
        return keeps, 1.0
    raise ValueError(profile)


def make_inputs(case):
    """(ids int64 [B, L], 13 fp32 parameters, keeps or None, scale, dpooled fp32 [B, 256])."""
    seed, B, L, pads, dp, kp, pp = case
    keeps, scale = make_keeps(seed, B, L, kp)
    dpooled = torch.randn((B, C), generator=torch.Generator().manual_seed(1000 + seed)) * GP.factors(dp, B, 1, C).squeeze(1)
    return make_ids(seed, B, L, pads), make_params(seed, pp), keeps, scale, dpooled.contiguous()


# ------------------------------------------------------------------------------------------------------------- the op
DEFECTS = ("small_row", "m_covered", "dz_uncovered", "dz_unchosen", "across_reads", "last_chunk", "dt_stale", "outside_counted", "once_lost", "no_eps",
           "no_mask_scale")


def _cdf(u):
    """The normal cdf as 0.5 erfc(-u / sqrt 2), as the kernels take it (csrc/clm_common.h normal_cdf): 0.5 (1 + erf) is a multiple of
    2^-25 in float32 and of 2^-54 in float64, and under `dead` (u near -6, cdf 1e-9) that left y, the choice among such values, dy
    and every sum over dy of the odd channels good to a few per cent in ANY float32 evaluation -- the yardstick read 3.4e-2 there."""
    return 0.5 * torch.special.erfc(u * -0.7071067811865476)


def _gelu(u):
    return u * _cdf(u)


def _gelu_grad(u):
    return _cdf(u) + u * 0.3989422804014327 * torch.exp(-0.5 * u * u)


def _shift(x, s: int, leak: bool = False):
    """out[b, t] = x[b, t + s], 0 outside the read (`leak`: the reads as one sequence, a tap reaches the neighbouring read)."""
    if s == 0:
        return x
    B, L, _ = x.shape
    if leak:
        flat = x.reshape(1, B * L, -1)
        return _shift(flat, s).reshape(x.shape)
    out = torch.zeros_like(x)
    if s > 0:
        out[:, :L - s] = x[:, s:]
    else:
        out[:, -s:] = x[:, :L + s]
    return out


def _conv(x, W, bias, second=False):
    """z[b, t, co] = bias + sum_k x[b, t + k - 3] . W[co, :, k], one product per tap, the taps added in order."""
    if second:
        return F.conv1d(x.transpose(1, 2), W, bias, padding=HALO).transpose(1, 2).contiguous()
    z = None
    for k in range(KW):
        t = _shift(x, k - HALO) @ W[:, :, k].T
        z = t if z is None else z + t
    return z if bias is None else z + bias


def _conv_t(dz, W, leak=False):
    """dx[b, t, ci] = sum_k dz[b, t - k + 3] . W[:, ci, k]."""
    dx = None
    for k in range(KW):
        t = _shift(dz, HALO - k, leak) @ W[:, :, k]
        dx = t if dx is None else dx + t
    return dx


def _dw(dz, x, leak=False, second=False):
    """dW[co, ci, k] = sum_{b, t} dz[b, t, co] x[b, t + k - 3, ci]."""
    a = dz.reshape(-1, C)
    taps = []
    for k in range(KW):
        xs = _shift(x, k - HALO, leak).reshape(-1, C)
        if second:                                                     # per 1,000 positions, the partials added in order
            t = sum(a[r:r + 1000].T @ xs[r:r + 1000] for r in range(0, a.shape[0], 1000))
        else:
            t = a.T @ xs
        taps.append(t)
    return torch.stack(taps, dim=2)


def _colsum(v, min_chunk=STAT_MIN, second=False, drop_last=False):
    """Column sums of v [B, n, 256] over all rows.  `second`: per 1,000 rows, the partials added in order; `drop_last`: the defect
    of a last short workgroup of ct_split's grid left out."""
    v = v.reshape(-1, v.shape[-1])
    n = v.shape[0]
    if drop_last:
        chunk, grid = ct_split(n, STAT_GRID, min_chunk)
        if n % chunk:
            v = v[:(grid - 1) * chunk]
    if second:
        return sum(v[r:r + 1000].sum(0) for r in range(0, v.shape[0], 1000))
    return v.sum(0)


def evaluate(inp, dtype, choice=None, defect=None, second=False) -> dict:
    """forward + backward of the op in `dtype` on the CPU, routed by `choice` (three [B, L_{i+1}, 256] arrays; None: the evaluation's
    own first maximum).  Keys: z{i}, y{i}, mean{i}, var{i}, dz{i}, dW{i}, db{i}, dg{i}, dbeta{i} (i = 0, 1, 2), pooled, dE, `choice` (three
    int64 tensors) and `den` {key: denominator} for the keys that have one.  `second`: the same formulas with every long sum split
    another way (a library convolution; column sums, dW and dT per 1,000 positions).  `defect`: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    ids, params, keeps, scale, dpooled = inp
    P = [p.to(dtype) for p in params]
    E, W, bias, g, beta = P[0], P[1::4], P[2::4], P[3::4], P[4::4]
    B, L = ids.shape
    Ls = lens(L)
    last = defect == "last_chunk"
    out, den = {}, {}
    idp = F.pad(ids, (HALO, HALO), value=VOC)                          # row 12: outside the read
    toks = torch.stack([idp[:, dk:dk + L] for dk in range(KW)], dim=2).reshape(B * L, KW)      # token under tap dk of every position
    km = [None if keeps is None else keeps[i].to(dtype) * scale for i in range(3)]
    xs, xhs, us, rstds, chs = [], [], [], [], []
    x = None
    for i in range(3):
        Lin, Lout, n = Ls[i], Ls[i + 1], B * Ls[i]
        if i == 0:
            table = torch.cat([torch.einsum("oik,ti->kto", W[0], E), torch.zeros(KW, 1, C, dtype=dtype)], dim=1)   # [7, 13, 256]
            z = bias[0].expand(B * L, C)
            for dk in range(KW):
                z = z + table[dk][toks[:, dk]]
            z = z.reshape(B, L, C)
        else:
            z = _conv(x, W[i], bias[i], second)
        mu = _colsum(z, second=second, drop_last=last) / n
        var = _colsum((z - mu) ** 2, second=second, drop_last=last) / n
        rstd = 1.0 / torch.sqrt(var if defect == "no_eps" else var + EPS)
        xh = (z - mu) * rstd
        u = g[i] * xh + beta[i]
        y = _gelu(u)
        win = y[:, :4 * Lout].reshape(B, Lout, 4, C)
        ch = win.argmax(2) if choice is None else torch.as_tensor(np.asarray(choice[i])).to(torch.int64)
        p = win.gather(2, ch[:, :, None, :]).squeeze(2)
        x = p if km[i] is None else p * km[i]
        out[f"z{i}"], out[f"y{i}"], out[f"mean{i}"], out[f"var{i}"] = z, y, mu, var
        den[f"mean{i}"] = _colsum(z.abs()) / n
        xs.append(x); xhs.append(xh); us.append(u); rstds.append(rstd); chs.append(ch)
    out["pooled"] = x.mean(1)
    out["choice"] = chs

    gin = (dpooled.to(dtype)[:, None, :] / Ls[3]).expand(B, Ls[3], C)
    gin_abs = gin.abs()
    for i in (2, 1, 0):
        Lin, Lout, n = Ls[i], Ls[i + 1], B * Ls[i]
        xh, rstd, ch4 = xhs[i], rstds[i], chs[i][:, :, None, :]
        mask = km[i]
        if mask is not None and defect == "no_mask_scale":
            mask = keeps[i].to(dtype)
        gi, gi_abs = (gin, gin_abs) if mask is None else (gin * mask, gin_abs * mask)
        gp = _gelu_grad(us[i][:, :4 * Lout].reshape(B, Lout, 4, C).gather(2, ch4).squeeze(2))
        xhc = xh[:, :4 * Lout].reshape(B, Lout, 4, C).gather(2, ch4).squeeze(2)
        dyc, dyc_abs = gi * gp, gi_abs * gp.abs()
        s1 = _colsum(dyc, DY_MIN, second, last)
        s2 = _colsum(dyc * xhc, DY_MIN, second, last)
        out[f"dbeta{i}"], out[f"dg{i}"] = s1, s2
        den[f"dbeta{i}"], den[f"dg{i}"] = _colsum(dyc.abs()), _colsum((dyc * xhc).abs())
        nn = B * 4 * Lout if defect == "m_covered" else n
        m1, m2 = s1 / nn, s2 / nn
        dy, dy_abs = torch.zeros(B, Lin, C, dtype=dtype), torch.zeros(B, Lin, C, dtype=dtype)
        dy[:, :4 * Lout].unflatten(1, (Lout, 4)).scatter_(2, ch4, dyc[:, :, None, :])
        dy_abs[:, :4 * Lout].unflatten(1, (Lout, 4)).scatter_(2, ch4, dyc_abs[:, :, None, :])
        dz = g[i] * rstd * (dy - m1 - xh * m2)
        den[f"dz{i}"] = (g[i].abs() * rstd * (dy_abs + m1.abs() + (xh * m2).abs())).amax(-1)
        if defect == "dz_uncovered":
            dz[:, 4 * Lout:] = 0
        if defect == "dz_unchosen":
            chosen = torch.zeros(B, Lin, C, dtype=torch.bool)
            chosen[:, :4 * Lout].unflatten(1, (Lout, 4)).scatter_(2, ch4, torch.ones_like(ch4, dtype=torch.bool))
            dz = dz * chosen
        del dy, dy_abs
        out[f"dz{i}"] = dz
        out[f"db{i}"], den[f"db{i}"] = _colsum(dz, second=second, drop_last=last), _colsum(dz.abs())
        if i > 0:
            leak = defect == "across_reads"
            out[f"dW{i}"] = _dw(dz, xs[i - 1], leak, second)
            if defect == "small_row" and i == 2:                        # the dW_2 rows of the channels c mod 13 = 12 lose their last tap
                out[f"dW{i}"][12::13, :, KW - 1] = 0
            den[f"dW{i}"] = _dw(dz.abs(), xs[i - 1].abs()).amax(1)                     # [co, tap]
            gin, gin_abs = _conv_t(dz, W[i], leak), _conv_t(dz.abs(), W[i].abs())
        else:
            flat = dz.reshape(B * L, C)
            tk = toks
            if defect == "dt_stale":                                   # the second stretch of a workgroup's chunk walks the first's rows
                chunk, _ = ct_split(B * L, DT_GRID, DT_MIN)
                r = torch.arange(B * L)
                idx = r % chunk
                tk = toks[torch.where(idx >= DT_SUB, r - DT_SUB, r)]
            dT = torch.zeros(KW, VOC + 1, C, dtype=dtype)
            for dk in range(KW):                                       # (a running float32 sum over 10^5 positions would be the worse yardstick)
                if second:                                             # per 1,000 positions as a product with the one-hot rows
                    hot = F.one_hot(tk[:, dk], VOC + 1).to(dtype)
                    dT[dk] = sum(hot[r:r + 1000].T @ flat[r:r + 1000] for r in range(0, B * L, 1000))
                else:
                    for tok in range(VOC + 1):
                        dT[dk, tok] = flat[tk[:, dk] == tok].sum(0)
            if defect == "outside_counted":
                dT[:, 11] += dT[:, VOC]
            dT = dT[:, :VOC]
            out["dW0"] = torch.einsum("kto,ti->oik", dT, E)
            absT = torch.zeros(KW, VOC + 1, C, dtype=dtype)
            for dk in range(KW):
                absT[dk].index_add_(0, toks[:, dk], flat.abs())
            den["dW0"] = torch.einsum("kto,ti->oik", absT[:, :VOC], E.abs()).amax(1)
            dE = torch.einsum("kto,oik->ti", dT, W[0])
            dE_abs = torch.einsum("kto,oik->ti", dT.abs(), W[0].abs())
            dE[PAD], dE_abs[PAD] = 0, 0
            if defect == "once_lost":
                dE[0] = 0
            out["dE"], den["dE"] = dE, dE_abs.amax(1)
    out["den"] = den
    return out


@lru_cache(maxsize=2)
def host_case(case):
    """(inputs, float64 reference, float32 yardstick), both routed by the YARDSTICK's own choice: the host tests' engine-free case."""
    inp = make_inputs(case)
    r32 = evaluate(inp, torch.float32)
    return inp, evaluate(inp, torch.float64, choice=r32["choice"]), r32


GRAD_KEYS = ["dE"] + [f"{k}{i}" for i in range(3) for k in ("dW", "db", "dg", "dbeta")]           # the ABI's order of the 13 gradients


# ------------------------------------------------------------------------------------------------------------- rows
def rows(ev, r64, L: int):
    """[(output, statistic, locate)] of an evaluation `ev` (the keys of `evaluate`) against r64."""
    Ls = lens(L)
    den = r64["den"]
    res = []

    def at(i):
        def locate(b, t):
            Lin, Lout = Ls[i], Ls[i + 1]
            w = f"window {t // 4} of {Lout}" if t < 4 * Lout else f"past 4 L_out = {4 * Lout}: no window covers it"
            n = b * Lin + t
            where = f"read {b} position {t} of {Lin} ({w}); row {n} of {ev[f'z{i}'].shape[0] * Lin}, 64-row tile {t // 64} of the read"
            if i == 0:
                chunk, _ = ct_split(ev["z0"].shape[0] * Lin, DT_GRID, DT_MIN)
                where += f", dt workgroup {n // chunk} position {n % chunk} of its {chunk}"
            return where
        return locate

    chan = lambda b, c: f"channel {c}"                                                 # noqa: E731
    for i in range(3):
        res.append((f"z{i}", G._stat(ev[f"z{i}"], r64[f"z{i}"]), at(i)))
        res.append((f"y{i}", G._stat(ev[f"y{i}"], r64[f"y{i}"]), at(i)))
        res.append((f"mean{i}", G._stat(ev[f"mean{i}"].reshape(1, C, 1), r64[f"mean{i}"].reshape(1, C, 1), den[f"mean{i}"].reshape(1, C)), chan))
        res.append((f"var{i}", G._stat(ev[f"var{i}"].reshape(1, C, 1), r64[f"var{i}"].reshape(1, C, 1)), chan))
    res.append(("pooled", G._stat(ev["pooled"][:, None], r64["pooled"][:, None]), lambda b, _: f"read {b}"))
    for i in (2, 1, 0):
        res.append((f"dz{i}", G._stat(ev[f"dz{i}"], r64[f"dz{i}"], den[f"dz{i}"]), at(i)))
        cut = lambda t: t.permute(0, 2, 1).reshape(1, C * KW, C)                      # noqa: E731  row = co * 7 + tap
        res.append((f"dW{i}", G._stat(cut(ev[f"dW{i}"]), cut(r64[f"dW{i}"]), den[f"dW{i}"].reshape(1, C * KW)),
                    lambda b, r: f"co {r // KW} tap {r % KW}"))
        for k in ("dg", "dbeta", "db"):
            res.append((f"{k}{i}", G._stat(ev[f"{k}{i}"].reshape(1, C, 1), r64[f"{k}{i}"].reshape(1, C, 1), den[f"{k}{i}"].reshape(1, C)), chan))
    res.append(("dE", G._stat(ev["dE"][None], r64["dE"][None], den["dE"][None]), lambda b, t: f"token {t}"))
    return res


def old_gates(ev, r64, r32):
    """[(output, error, bound)] of the tensor-wide gate of tests/test_gpu_cnn_train.py on every tensor it holds (db_i against dbeta_i's
    scale, as there)."""
    res = [(k,) + G.old_gate(ev[k], r64[k], r32[k]) for k in ["pooled", "dE"] + [f"{s}{i}" for i in range(3) for s in ("z", "mean", "var", "dz", "dW", "dg", "dbeta")]]
    for i in range(3):
        _, bound = G.old_gate(r32[f"dbeta{i}"], r64[f"dbeta{i}"], r32[f"dbeta{i}"])
        res.append((f"db{i}", float(ev[f"db{i}"].abs().max()) / float(r64[f"dbeta{i}"].abs().max()), bound))
    return res


# ------------------------------------------------------------------------------------------------------------- the choice
def choice_report(choice, r64, r32, K, L: int):
    """Per block: (windows, of them differing, windows breaking the gap rule, exact float64 ties decided another way) of `choice` against the first maximum of r64's y (module docstring)."""
    Ls = lens(L)
    res = []
    for i in range(3):
        Lout = Ls[i + 1]
        y64, y32 = r64[f"y{i}"], r32[f"y{i}"]
        B = y64.shape[0]
        ch = torch.as_tensor(np.asarray(choice[i])).to(torch.int64)[:, :, None, :]
        win = y64[:, :4 * Lout].reshape(B, Lout, 4, C)
        first = win.argmax(2, keepdim=True)
        differ = (ch != first).squeeze(2)
        gap = (win.gather(2, first) - win.gather(2, ch)).squeeze(2)
        tol = torch.maximum(K * (y32.double() - y64).abs().amax((0, 1)), FLOOR * y64.abs().amax((0, 1)))
        res.append((differ.numel(), int(differ.sum()), int((differ & (gap > tol)).sum()), int((differ & (gap == 0)).sum())))
    return res


def choice_lines(tag, report):
    return [f"CHOICE {tag} block {i}: {n} windows, {d} of them differ ({d / max(n, 1):.2e}); "
            f"{v} break the gap rule; {t} exact float64 ties decided another way" for i, (n, d, v, t) in enumerate(report)]


def choice_ok(report) -> bool:
    return all(d <= DIFFER_CAP * n and v == 0 and t == 0 for n, d, v, t in report)
