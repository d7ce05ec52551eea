"""The SequenceCNNTransformer forward (csrc/tf_fp32.hip + tail32.hip; csrc/tf_model.hip) stage by stage, in plain torch, for
tests/test_gpu_tf_stages.py and tests/test_tf_stage_host.py.  Written from oracle/transformer_oracle.py's formulas.

One function per stage, each mapping that stage's INPUT to its output in the dtype of the input: evaluated in float64 on the engine's
own fetched input it is the reference of that stage alone (an error made upstream does not count against it); evaluated in float32 on
the CPU on the same input it is the yardstick of the exact modes, the error the same formulas have in the engine's number format.
`lin` replaces the plain product a @ W^T of a stage (the fp16x3 split model, tests/error_model.py x3_linear).  `fmt` makes a stage the
MODEL of its 16-bit kernel: the same stage in float64, rounding where the kernel rounds (tests/error_model.py rnd):
    * embedding rows are rounded to the element type when the first stem kernel stages them (to_bits in conv3_relu_pool_kernel<., true>);
    * weights are rounded as packed: fp16 / bf16, or fp16c's fp16 hi + e4m3-grade lo ("h8"), every matrix and every stem tap alike;
    * accumulation, bias, ReLU, max-pool, LayerNorm, the residual and the softmax pooling are fp32 (here: float64, unrounded);
    * every stored activation (x1, x2, x3, hx, qkv) is rounded once on store;
    * the layer kernel (enc_ffn16_kernel): x1 = LN1(..) is rounded as fc1's operand and kept unrounded as the residual; relu(fc1 + b1) is
      rounded into the LDS tile fc2 reads; the next layer's in_proj reads the rounded LN2 tile (= hx); fp16c sums the out_proj of the
      attention's two planes and multiplies by 1 / 64.
Not modelled (as in error_model.py): fp16c's lo product reads the activation truncated to e5m2 (a few per cent of a 2^-11 term), and
the fp32 arithmetic of the kernels themselves (two orders below a 16-bit rounding).  With EXACT every rounding is the identity and
each model IS the plain stage, bit for bit (tests/test_tf_stage_host.py).

Stages and the buffers they connect (clm_tf_debug_fetch names, include/chimeralm_hip.h):
    embed        ids                  -> "x0"  [B, L, 256]       (exact path; bit-equal to embedding.weight[ids])
    stem_level   rows [B, Lin, 256]   -> "x1" / "x2" / "x3"      Conv1d(k 3, padding 1) + ReLU + MaxPool1d(2, 2): [B, Lin // 2, 256]
    pe_ln        "x3"                 -> "hidden" (and "hx")     + positional encoding, LayerNorm
    in_proj      "hidden"             -> "qkv" [B, L3, 768]
    attention    "qkv"                -> "att" [B, L3, 256]
    layer_tail   "hidden", "att"      -> "hidden"                LN2(x1 + W_2 relu(W_1 x1 + b_1) + b_2), x1 = LN1(h + W_o att + b_o)
    pool_scores / pooled / logits   "hidden" -> "scores" [B, L3], "pooled" [B, 256], logits [B, 2]
`statistic`, `read_stats` and `check` are the comparison the tests share.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from error_model import rnd

D, NH, HD = 256, 8, 32
EPS = 1e-5
FLOOR = 32 * 2.0 ** -24            # the project's floor (tests/test_gpu_headtrain.py)


@dataclass(frozen=True)
class Fmt:
    """Where a 16-bit kernel rounds: `act` stored activations and GEMM operands, `w` packed weights (error_model.rnd modes),
    `hilo` the attention output as the two planes fp16(64 a), fp16(64 a - hi)."""
    act: str | None = None
    w: str | None = None
    hilo: bool = False


EXACT = Fmt()
FORMATS = {"fp16": Fmt("h", "h"), "bf16": Fmt("b", "b"), "fp16c": Fmt("h", "h8", True)}
HILO_SCALE = 64.0


def weights(sd: dict, dtype, device="cpu") -> dict:
    return {k: v.detach().to(device, dtype) for k, v in sd.items()}


def n_layers_of(sd: dict) -> int:
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_encoder.layers."))


def _p(i: int) -> str:
    return f"transformer_encoder.layers.{i}."


def _mm(a, W, fmt: Fmt, lin):
    return lin(a, W) if lin is not None else a @ rnd(W, fmt.w).T


# ------------------------------------------------------------------------------------------------------------- the stages
def embed(w: dict, ids: torch.Tensor) -> torch.Tensor:
    return w["embedding.weight"][ids]


def stem_level(w: dict, c: int, x: torch.Tensor, fmt: Fmt = EXACT, lin=None) -> torch.Tensor:
    """Level c (0, 1, 2) of the stem on the rows x [B, Lin, 256]: [B, Lin // 2, 256]; a trailing odd position is dropped by the pooling,
    whose last kept output still saw it as its right neighbour."""
    W, b = w[f"cnn.{3 * c}.weight"], w[f"cnn.{3 * c}.bias"]
    x = rnd(x, fmt.act)                                        # (level 0: the embedding rows as staged; later levels: already 16-bit)
    if lin is None:
        y = F.conv1d(x.transpose(1, 2), rnd(W, fmt.w), b, padding=1).transpose(1, 2)
    else:                                                      # the three taps as products over the zero-padded rows
        xp = F.pad(x, (0, 0, 1, 1))
        Lin = x.shape[1]
        y = sum(lin(xp[:, dk:dk + Lin], W[:, :, dk]) for dk in range(3)) + b
    y = F.max_pool1d(F.relu(y).transpose(1, 2), 2, 2).transpose(1, 2)
    return rnd(y, fmt.act)


def pe_ln(w: dict, x3: torch.Tensor) -> torch.Tensor:
    """The residual stream in front of layer 0 (fp32 in every mode; "hx" is it rounded once)."""
    x = x3 + w["pos_encoder.pe"][:, :x3.shape[1]]
    return F.layer_norm(x, (D,), w["norm.weight"], w["norm.bias"], EPS)


def in_proj(w: dict, i: int, h: torch.Tensor, fmt: Fmt = EXACT, lin=None) -> torch.Tensor:
    p = _p(i)
    return rnd(_mm(rnd(h, fmt.act), w[p + "self_attn.in_proj_weight"], fmt, lin) + w[p + "self_attn.in_proj_bias"], fmt.act)


def attention(qkv: torch.Tensor) -> torch.Tensor:
    """softmax(q k^T / sqrt(32)) v per read and head, no mask: [B, L3, 768] -> [B, L3, 256]."""
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, NH, HD).transpose(1, 2) for t in qkv.split(D, dim=-1))
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(HD)
    return torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, L, D)


def attention_x3(qkv: torch.Tensor) -> torch.Tensor:
    """The fp16x3 FORMAT's attention (attention_x3_kernel), in float64: q, k, v and the unnormalised probabilities p = exp(s - max s)
    each as hi = fp16(x), lo = fp16(x - hi), unscaled, and the three products hi hi + lo hi + hi lo.  A v (or p) below 2^-14 has
    its lo half, and at last its hi half, in fp16's subnormal range: an absolute 2^-25 instead of a relative 2^-22.  Not modelled: the
    running maximum of the online softmax (p is taken against the final one) and the fp32 sums."""
    from error_model import x3_split

    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, NH, HD).transpose(1, 2).double() for t in qkv.split(D, dim=-1))
    (qh, ql), (kh, kl), (vh, vl) = x3_split(q), x3_split(k), x3_split(v)
    s = (qh @ (kh + kl).transpose(-1, -2) + ql @ kh.transpose(-1, -2)) / math.sqrt(HD)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    ph, pl = x3_split(p)
    o = (ph @ (vh + vl) + pl @ vh) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, L, D)


def layer_tail(w: dict, i: int, h: torch.Tensor, att, fmt: Fmt = EXACT, lin=None, trace: dict | None = None) -> torch.Tensor:
    """Everything of layer i behind its attention.  `att`: [B, L3, 256], or for a `hilo` format the pair of planes (hi, lo)."""
    p = _p(i)
    Wo = w[p + "self_attn.out_proj.weight"]
    if fmt.hilo:
        o = (_mm(att[0], Wo, fmt, lin) + _mm(att[1], Wo, fmt, lin)) * (1.0 / HILO_SCALE)
    else:
        o = _mm(att, Wo, fmt, lin)
    x1 = F.layer_norm(h + o + w[p + "self_attn.out_proj.bias"], (D,), w[p + "norm1.weight"], w[p + "norm1.bias"], EPS)
    u = rnd(F.relu(_mm(rnd(x1, fmt.act), w[p + "linear1.weight"], fmt, lin) + w[p + "linear1.bias"]), fmt.act)
    f = _mm(u, w[p + "linear2.weight"], fmt, lin) + w[p + "linear2.bias"]
    if trace is not None:
        trace.update(x1=x1, ffn=f)
    return F.layer_norm(x1 + f, (D,), w[p + "norm2.weight"], w[p + "norm2.bias"], EPS)


def pool_scores(w: dict, h: torch.Tensor) -> torch.Tensor:
    return (h @ w["attn_pool.weight"].T)[..., 0] + w["attn_pool.bias"]


def pooled(w: dict, h: torch.Tensor) -> torch.Tensor:
    a = torch.softmax(pool_scores(w, h), dim=1)
    return (a[..., None] * h).sum(dim=1)


def logits(w: dict, pooled_rows: torch.Tensor) -> torch.Tensor:
    x = F.relu(F.linear(pooled_rows, w["classifier.0.weight"], w["classifier.0.bias"]))
    return F.linear(x, w["classifier.3.weight"], w["classifier.3.bias"])


def forward(sd: dict, ids, dtype=torch.float64, fmt: Fmt = EXACT, trace: dict | None = None) -> torch.Tensor:
    """Logits of the net chained from the stages (tests/test_tf_stage_host.py holds it to the oracle); `trace` receives every buffer
    under the oracle's trace names and the engine's fetch names."""
    w = weights(sd, dtype)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    tr = {} if trace is None else trace
    x = tr["x0"] = embed(w, ids)
    for c in range(3):
        x = tr[f"x{c + 1}"] = tr[f"cnn{c}"] = stem_level(w, c, x, fmt)
    h = tr["embedded"] = pe_ln(w, x)
    for i in range(n_layers_of(sd)):
        qkv = tr[f"qkv{i}"] = in_proj(w, i, h, fmt)
        a = tr[f"att{i}"] = attention(qkv)
        if fmt.hilo:
            hi = rnd(a * HILO_SCALE, fmt.act)
            a = (hi, rnd(a * HILO_SCALE - hi, fmt.act))
        else:
            a = rnd(a, fmt.act)
        h = tr[f"layer{i}"] = layer_tail(w, i, h, a, fmt)
    tr["scores"] = pool_scores(w, h)
    tr["pool_weights"] = torch.softmax(tr["scores"], dim=1)[..., None]
    tr["pooled"] = pooled(w, h)
    return logits(w, tr["pooled"])


# ------------------------------------------------------------------------------------------------------------- the comparison
def statistic(got, ref, den=None) -> torch.Tensor:
    """The per-position error [B, n] (float64) of `got` against the float64 `ref`.
      rows [B, n, C]:   max_c |got - ref| / max_c |ref|, the position's own row maximum as denominator;
      `den` [B] given:  |got - ref| / den[b] per entry of [B, n] (the pooling scores, over the read's max |score|);
      `den` [B, n] given with rows [B, n, C]:  max_c |got - ref| / den[b, n], a row's own sum of absolute terms (tests/grad_rows.py).
    A zero denominator demands an exact result: 0 where got == ref, inf elsewhere."""
    got, ref = got.double(), ref.double()
    diff = (got - ref).abs()
    if den is None:
        num, d = diff.amax(-1), ref.abs().amax(-1)
    elif den.dim() == 2:
        num, d = diff.amax(-1), den.double()
    else:
        num, d = diff, den.double()[:, None].expand_as(diff)
    return torch.where(d > 0, num / d.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))))


def read_stats(stat: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """Per read: (max, rms) over the positions of a per-position statistic [B, n]."""
    return stat.amax(1).cpu().numpy(), stat.pow(2).mean(1).sqrt().cpu().numpy()


def where(b: int, t: int, n: int, tile: int | None) -> str:
    """The code path a position belongs to, for a failure message (`tile`: rows per tile of the flattened [B * n] rows)."""
    s = f"read {b} position {t} of {n}" + (", the last" if t == n - 1 else "") + (", the first" if t == 0 else "")
    if tile:
        m = b * n + t
        s += f"; flattened row {m}: tile {m // tile} of {tile} rows, row {m % tile} in it"
    return s


def check(tag: str, stage: str, eng: torch.Tensor, yard: torch.Tensor, K: float | None, rows: list, bad: list,
          tile: int | None = None) -> tuple[float, float]:
    """Holds the engine's per-position statistic to max(K x the yardstick's, FLOOR), per read, for the max and the rms over positions
    (K None: measures only).  Appends one printed line per (read, statistic) to `rows` and the failing ones to `bad`, naming the worst
    position.  Returns the worst engine / yardstick ratio (0 / 0 counting as 0): (over all figures, over those above the floor)."""
    worst, worst_above = 0.0, 0.0
    e_max, e_rms = read_stats(eng)
    y_max, y_rms = read_stats(yard)
    n = eng.shape[1]
    for b in range(eng.shape[0]):
        t = int(eng[b].argmax())
        for name, e, y in (("max", e_max[b], y_max[b]), ("rms", e_rms[b], y_rms[b])):
            ratio = 0.0 if e == 0 else float(e) / float(y) if y > 0 else float("inf")
            worst = max(worst, ratio)
            if e > FLOOR or not np.isfinite(e):
                worst_above = max(worst_above, ratio)
            bound = float("inf") if K is None else max(K * y, FLOOR)
            line = (f"{tag:40s} {stage:10s} read {b} {name}: engine {e:.3e}  yardstick {y:.3e}  ratio {ratio:8.2f}  bound {bound:.3e}  "
                    f"worst: {where(b, t, n, tile)}")
            rows.append(line)
            if not (np.isfinite(e) and e <= bound):
                bad.append(line)
    return worst, worst_above


# ------------------------------------------------------------------------------------------------------------- nets and regimes
def make_net(seed: int, layers: int = 1, max_len: int = 512) -> dict:
    """A seeded d 256 net of `layers` encoder layers (oracle.transformer_oracle.make_state_dict; a short `pos_encoder.pe`)."""
    from oracle import transformer_oracle as to

    return to.make_state_dict(seed, to.Config(num_encoder_layers=layers, max_len=max_len), scale=1.0)


def _scale_rows(sd: dict, rows: slice, s: float, i: int = 0) -> None:
    for k in ("self_attn.in_proj_weight", "self_attn.in_proj_bias"):
        t = sd[_p(i) + k].clone()
        t[rows] *= s
        sd[_p(i) + k] = t


Q_ROWS, K_ROWS, V_ROWS = slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)
# The issue's regimes: dead channels | peaked and flat attention | sublayer scale (two settings) | peaked pooling.  fp32 and fp16x3 run
# all of them; fp16c and fp16 run the first three, REGIMES_16 (the sublayer scale is what stresses enc_ffn16_kernel's out_proj sum onto
# the residual, fp16c's two planes and their 1 / 64 included).
REGIMES = ("dead", "peaked", "flat", "sub2^-6", "subx8", "pool16")
REGIMES_16 = REGIMES[:5]
V_SCALES = (0, 4, 8, 12)                                               # fp16x3 activation scale: the v rows of in_proj x 2^-k


def regime_state_dict(regime: str, seed: int = 60) -> dict:
    """A one-layer net pushed into a regime through its weights:
    dead     cnn.*.bias = -10 on the odd channels: exact zeros through the stem, LayerNorm on rows that are half zero;
    peaked   the q and k rows of in_proj (weights and biases) x 8: near one-hot attention;
    flat     the q rows x 0: every weight 1 / L3, att = the mean of v, small against h;
    sub2^-6, subx8   out_proj.weight and linear2.weight x 2^-6, x 8: the sublayers small against / large over the residual;
    pool16   attn_pool.weight x 16: a peaked pooling softmax;
    v2^-k    the v rows of in_proj x 2^-k: a small att under an order-1 stream (the fp16x3 activation-scale axis)."""
    sd = make_net(seed)
    if regime == "dead":
        for c in (0, 3, 6):
            b = sd[f"cnn.{c}.bias"].clone()
            b[1::2] = -10.0
            sd[f"cnn.{c}.bias"] = b
    elif regime == "peaked":
        _scale_rows(sd, Q_ROWS, 8.0)
        _scale_rows(sd, K_ROWS, 8.0)
    elif regime == "flat":
        _scale_rows(sd, Q_ROWS, 0.0)
    elif regime in ("sub2^-6", "subx8"):
        s = 2.0 ** -6 if regime == "sub2^-6" else 8.0
        for k in ("self_attn.out_proj.weight", "linear2.weight"):
            sd[_p(0) + k] = sd[_p(0) + k] * s
    elif regime == "pool16":
        sd["attn_pool.weight"] = sd["attn_pool.weight"] * 16.0
    elif regime.startswith("v2^-"):
        _scale_rows(sd, V_ROWS, 2.0 ** -int(regime[4:]))
    else:
        raise ValueError(regime)
    return sd


def stage_ids(seed: int, B: int, L: int) -> np.ndarray:
    """Read 0 left-padded to its last token with [PAD], read 1 without pads, read 2 with 3 pads and one N."""
    from oracle import transformer_oracle as to

    ids = to.synthetic_ids(seed, B, L)
    ids[ids == 11] = 7                                         # (the one N is placed, not drawn)
    ids[0, :L - 1] = 4
    if B > 2:
        ids[2, :3] = 4
        ids[2, L // 2] = 11
    return ids
