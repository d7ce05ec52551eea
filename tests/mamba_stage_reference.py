"""The Mamba inference forward (csrc/mamba.hip) stage by stage, in plain torch, for tests/test_gpu_mamba_stages.py.

One function per stage, each mapping that stage's INPUT to its output in the dtype of the input: evaluated in float64 on the engine's
own fetched input it is the reference of that stage alone (an error made upstream does not count against it); evaluated in float32 on
the CPU on the same input it is the yardstick, the error the same formulas have in the engine's number format (the idea of
tests/mamba_train_reference.py).  The scan is `mamba_reference.scan_chunked` at Q = 64 in both: it is the arithmetic the kernel and
`mamba_ssm` use, and the sequential recurrence does not have its s_i - s_j cancellation.

Stages and the `clm_mamba_debug_fetch` names they connect (the last layer's workspace; see include/chimeralm_hip.h):
    front     ids (, mask)            -> "front"  [B, L, d]
    in_proj   h                       -> "zx"     [B, L, n_in_pad]: z | x | B | C | softplus(dt + dt_bias) | zeros
    conv      zx                      -> "xc"     [B, L, di + 2 N]
    scan      zx, xc                  -> "g"      [B, L, di], "ssq" [B, L, H]
    out_proj  h, g, ssq (, mask)      -> the next residual rows ("layer0" of a one-layer net)
    partials  rows                    -> "part"   [B, ceil(L / 64), 2, d]
`statistic`, `token_stats` and `check` are the comparison the GPU tests share.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from mamba_reference import D_CONV, HEADDIM, _layer_prefix, make_mamba_state_dict, scan_chunked

EPS = 1e-5
TILE = 64
FLOOR = 32 * 2.0 ** -24            # the floor of tests/test_gpu_mamba_train.py


@dataclass(frozen=True)
class Dims:
    d: int
    di: int
    H: int
    N: int

    @property
    def conv_dim(self):
        return self.di + 2 * self.N

    @property
    def n_in(self):
        return 2 * self.di + 2 * self.N + self.H

    @property
    def n_in_pad(self):
        return (self.n_in + 255) // 256 * 256

    @property
    def dt0(self):
        return 2 * self.di + 2 * self.N


def n_layers_of(sd: dict) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("mamba_layers."))


def layer_params(variant: str, sd: dict, i: int, dtype, device="cpu") -> dict:
    pre = _layer_prefix(variant, i)
    return {k[len(pre):]: v.detach().to(device, dtype) for k, v in sd.items() if k.startswith(pre)}


def dims_of(p: dict) -> Dims:
    H = p["A_log"].shape[0]
    di = p["norm.weight"].shape[0]
    return Dims(d=p["in_proj.weight"].shape[1], di=di, H=H, N=(p["conv1d.bias"].shape[0] - di) // 2)


# ------------------------------------------------------------------------------------------------------------- the stages
def front_pre(variant: str, w: dict, ids: torch.Tensor) -> torch.Tensor:
    """What the front's product sees: E[id] (+ pos for `mamba`), in the dtype of `w`."""
    h = F.embedding(ids, w["embedding.weight"])
    if variant == "mamba":
        h = h + w["pos_embedding"][:, :ids.shape[1]]
    return h


def front_post(variant: str, w: dict, y: torch.Tensor | None, pre: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    """`mamba`: bias, LayerNorm and mask on the Linear's product `y` (None: computed here); `mambasp`: the embedding itself."""
    if variant != "mamba":
        return pre
    if y is None:
        y = pre @ w["input_block.0.weight"].T
    h = F.layer_norm(y + w["input_block.0.bias"], (y.shape[-1],), w["input_block.1.weight"], w["input_block.1.bias"], eps=EPS)
    return h if mask is None else h * mask.to(h.dtype)[..., None]


def front(variant: str, w: dict, ids: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
    return front_post(variant, w, None, front_pre(variant, w, ids), mask)


def in_proj_post(p: dict, raw: torch.Tensor) -> torch.Tensor:
    """softplus(. + dt_bias) on the dt columns of the product `raw` [B, L, n_in]."""
    D = dims_of(p)
    return torch.cat([raw[..., :D.dt0], F.softplus(raw[..., D.dt0:] + p["dt_bias"])], dim=-1)


def in_proj(p: dict, h: torch.Tensor) -> torch.Tensor:
    """zx [B, L, n_in] (without the engine's zero padding)."""
    return in_proj_post(p, h @ p["in_proj.weight"].T)


def conv(p: dict, zx: torch.Tensor) -> torch.Tensor:
    """xc [B, L, conv_dim]: silu(causal depthwise conv + bias) of the x | B | C columns; rows before the read count as zero."""
    D = dims_of(p)
    L = zx.shape[1]
    xBC = zx[..., D.di:D.di + D.conv_dim]
    u = F.conv1d(xBC.transpose(1, 2), p["conv1d.weight"], p["conv1d.bias"], padding=D_CONV - 1, groups=D.conv_dim)[..., :L]
    return F.silu(u.transpose(1, 2))


def scan(p: dict, zx: torch.Tensor, xc: torch.Tensor, Q: int = 64):
    """(g [B, L, di], ssq [B, L, H]): the chunked scan, the D skip, the gate, the per-head sums of squares."""
    D = dims_of(p)
    Bn, L, _ = zx.shape
    z, dt = zx[..., :D.di], zx[..., D.dt0:D.dt0 + D.H]
    x, Bm, Cm = xc.split([D.di, D.N, D.N], dim=-1)
    A = -torch.exp(p["A_log"])
    y = scan_chunked(x.reshape(Bn, L, D.H, HEADDIM), dt, A, Bm, Cm, p["D"], Q=Q).reshape(Bn, L, D.di)
    g = y * F.silu(z)
    return g, g.reshape(Bn, L, D.H, HEADDIM).pow(2).sum(-1)


def out_weight(p: dict) -> torch.Tensor:
    """out_proj with norm.weight folded into its columns, as the engine packs it (the fold in float64, stored in p's dtype)."""
    return (p["out_proj.weight"].double() * p["norm.weight"].double()).to(p["out_proj.weight"].dtype)


def out_proj_post(p: dict, h_in, y, ssq, mask=None):
    """(h_in + y * rsqrt(sum ssq / d_inner + eps)) * mask on the product y = g @ out_weight^T."""
    D = dims_of(p)
    h = h_in + y * torch.rsqrt(ssq.sum(-1, keepdim=True) / D.di + EPS)
    return h if mask is None else h * mask.to(h.dtype)[..., None]


def out_proj(p: dict, h_in, g, ssq, mask=None):
    return out_proj_post(p, h_in, g @ out_weight(p).T, ssq, mask)


def partials(h: torch.Tensor) -> torch.Tensor:
    """part [B, ceil(L / 64), 2, d]: per 64-token tile the channel sums and maxima over the tile's rows."""
    out = []
    for t0 in range(0, h.shape[1], TILE):
        rows = h[:, t0:t0 + TILE]
        out.append(torch.stack([rows.sum(1), rows.max(1)[0]], dim=1))
    return torch.stack(out, dim=1)


def partial_scales(h: torch.Tensor) -> torch.Tensor:
    """The denominators of a tile's partials, [B, tiles, 2, d]: the sum of |rows| (what a channel sum cancels from) and max |rows|."""
    out = []
    for t0 in range(0, h.shape[1], TILE):
        rows = h[:, t0:t0 + TILE].abs()
        out.append(torch.stack([rows.sum(1), rows.max(1)[0]], dim=1))
    return torch.stack(out, dim=1)


def pooled_of(part: torch.Tensor, L: int) -> torch.Tensor:
    return (part[:, :, 0].sum(1) / L + part[:, :, 1].max(1)[0]) / 2


def head(w: dict, pooled: torch.Tensor) -> torch.Tensor:
    x = F.gelu(F.linear(pooled, w["pooler.0.weight"], w["pooler.0.bias"]))
    x = F.gelu(F.linear(x, w["classifier.0.weight"], w["classifier.0.bias"]))
    return F.linear(x, w["classifier.3.weight"], w["classifier.3.bias"])


def layer(p: dict, h, mask=None, trace: dict | None = None):
    """One whole layer from the stages: h -> the next residual rows."""
    zx = in_proj(p, h)
    xc = conv(p, zx)
    g, ssq = scan(p, zx, xc)
    if trace is not None:
        trace.update(zx=zx, xc=xc, g=g, ssq=ssq)
    return out_proj(p, h, g, ssq, mask)


def forward(variant: str, sd: dict, ids, mask=None, dtype=torch.float64, device="cpu", trace: dict | None = None) -> torch.Tensor:
    """Logits of the net composed from the stages (tests/test_mamba_stage_host.py holds it to `mamba_forward_fp64`)."""
    w = {k: v.detach().to(device, dtype) for k, v in sd.items()}
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64, device=device)
    m = None if mask is None or variant != "mamba" else torch.as_tensor(np.asarray(mask), dtype=dtype, device=device)
    h = front(variant, w, ids, m)
    for i in range(n_layers_of(sd)):
        tr = {} if trace is not None else None
        h = layer(layer_params(variant, sd, i, dtype, device), h, m, tr)
        if trace is not None:
            trace[i] = tr
    part = partials(h)
    if trace is not None:
        trace["part"] = part
    return head(w, pooled_of(part, ids.shape[1]))


# ------------------------------------------------------------------------------------------------------------- decay regimes
def regime_state_dict(regime: str, seed: int = 31) -> dict:
    """mambasp, one layer, d 256, expand 1, N 128, in a decay regime (set through dt_bias, A_log and the scale of in_proj's dt rows):
    flat   dt about 1e-4 ... 1e-3, A = 1: nothing decays, the state is a long sum;
    steep  dt up to about 2, A = 16: exp(s_i), w_j and exp(s_63) underflow inside a chunk;
    mixed  the default draw with in_proj's dt rows x 8: a head's dt swings over orders of magnitude from token to token."""
    sd = make_mamba_state_dict("mambasp", seed, n_layers=1, d_model=256, expand=1, d_state=128)
    H, dt_rows = 4, slice(2 * 256 + 2 * 128, 2 * 256 + 2 * 128 + 4)
    rng = np.random.default_rng(seed + 1)
    W = sd["mamba_layers.0.in_proj.weight"].clone()
    if regime == "mixed":
        W[dt_rows] *= 8.0
    else:
        lo, hi, A = {"flat": (1.5e-4, 6.5e-4, 1.0), "steep": (0.2, 2.0, 16.0)}[regime]
        dt = np.exp(rng.uniform(np.log(lo), np.log(hi), H))
        sd["mamba_layers.0.dt_bias"] = torch.from_numpy(dt + np.log(-np.expm1(-dt))).float()
        sd["mamba_layers.0.A_log"] = torch.full((H,), float(np.log(A)))
        W[dt_rows] *= 0.1
    sd["mamba_layers.0.in_proj.weight"] = W
    return sd


REGIMES = ("flat", "steep", "mixed")


# ------------------------------------------------------------------------------------------------------------- the comparison
def statistic(got, ref, kind: str = "row", groups: int = 1, den=None) -> torch.Tensor:
    """The per-token error [B, n] (float64) of `got` against the float64 `ref`, both [B, L, C]:
      "row"      max_c |got - ref| / max_c |ref|, the token's own row maximum as denominator; `groups` > 1 takes the numerator per
                 group of C / groups consecutive channels (per head: n = L x groups), the denominator stays the whole row's;
      "element"  |got - ref| / |ref| per element (n = L x C): the dt columns, which span orders of magnitude and each enter an exp;
      "den"      |got - ref| / den per element with a given denominator tensor (the pooling partials).
    A zero denominator demands an exact result: 0 where got == ref, inf elsewhere."""
    got, ref = got.double(), ref.double()
    diff = (got - ref).abs()
    Bn = ref.shape[0]
    if kind == "row":
        num = diff.reshape(Bn, ref.shape[1], groups, -1).amax(-1)
        d = ref.abs().amax(-1)[..., None].expand_as(num)
    elif kind == "element":
        num, d = diff, ref.abs()
    else:
        num, d = diff, den.double()
    out = torch.where(d > 0, num / d.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))))
    return out.reshape(Bn, -1)


def token_stats(stat: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """Per read: (max, rms) over the tokens of a per-token statistic [B, n]."""
    return stat.amax(1).cpu().numpy(), stat.pow(2).mean(1).sqrt().cpu().numpy()


def check(tag: str, stage: str, eng: torch.Tensor, yard: torch.Tensor, K: float, rows: list, bad: list, per: int = 1) -> float:
    """Holds the engine's per-token statistic to max(K x the yardstick's, FLOOR), per read, for the max and the rms over tokens.
    Appends one printed line per (read, statistic) to `rows` and the failing ones to `bad`; `per` entries of the statistic belong
    to one token (names the token in the message).  Returns the worst engine / yardstick ratio (0 / 0 counting as 0)."""
    worst = 0.0
    e_max, e_rms = token_stats(eng)
    y_max, y_rms = token_stats(yard)
    for b in range(eng.shape[0]):
        tok = int(eng[b].argmax()) // per
        for name, e, y in (("max", e_max[b], y_max[b]), ("rms", e_rms[b], y_rms[b])):
            bound = max(K * y, FLOOR)
            ratio = 0.0 if e == 0 else float(e) / max(float(y), 1e-300)
            worst = max(worst, ratio)
            line = (f"{tag:44s} {stage:12s} read {b} {name}: engine {e:.3e}  yardstick {y:.3e}  ratio {ratio:8.2f}  "
                    f"bound {bound:.3e}  worst token {tok}")
            rows.append(line)
            if not (np.isfinite(e) and e <= bound):
                bad.append(line)
    return worst
