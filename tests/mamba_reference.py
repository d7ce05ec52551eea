"""Seeded weights, a `Mamba2` parameter container and an independent fp64 forward for the tests of chimeralm_amd.mamba.

The reference's two Mamba nets (chimeralm/models/components/mamba.py: `MambaSequenceClassification`, `model: mamba`, and
`MambaSequenceClassificationSP`, `model: mambasp`) wrap `mamba_ssm.Mamba2`, a CUDA / Triton package.  Its forward is restated here
with the `mamba_ssm` 2.x defaults the reference uses (ngroups 1, gated RMSNorm with norm_before_gate False, D per head, no in_proj /
out_proj bias, conv bias, dt_limit (0, inf), zero initial state):

    [z | xBC | dt] = in_proj(u)                       widths d_inner, d_inner + 2 N, H
    xBC  = silu(causal depthwise conv, 4 taps, + bias) -> x (d_inner) | B (N) | C (N); head h owns x[:, hP:(h+1)P]
    dt   = softplus(dt + dt_bias), A = -exp(A_log)
    S_t  = exp(dt_t A) S_{t-1} + dt_t B_t x_t^T     (N x P per head);  y_t = C_t^T S_t + D x_t
    out  = out_proj(norm.weight * g * rsqrt(mean(g^2) + 1e-5)),  g = y * silu(z)

`scan_sequential` is that recurrence; `scan_chunked` is the chunk decomposition the HIP kernel implements (the tests hold the two to
1e-10).  `mamba_forward_fp64` is the whole net with the chunked scan; tests/golden/make_mamba_golden.py pins it to the reference's
own wrapper code (embedding, positional term, input block, masks, residuals, pooling, head) with `Mamba2` replaced by `Mamba2Ref`,
i.e. this container plus `scan_sequential`.  Mamba2's internals are thereby restated, not pinned.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

VOCAB, PAD, HEADDIM, D_CONV = 12, 4, 64, 4
VARIANTS = {
    # variant: (d_model, n_layers, d_state, expand, model_max_length or None)
    "mamba": (256, 12, 16, 2, 30000),
    "mambasp": (512, 3, 128, 3, None),
}


class Mamba2Ref(nn.Module):
    """`mamba_ssm.Mamba2`'s parameters (same names and shapes) and the sequential fp64 forward."""

    def __init__(self, d_model, d_state=128, d_conv=4, expand=2, headdim=64, **_):
        super().__init__()
        self.d_inner = expand * d_model
        self.nheads, self.headdim, self.d_state = self.d_inner // headdim, headdim, d_state
        conv_dim = self.d_inner + 2 * d_state
        self.in_proj = nn.Linear(d_model, 2 * self.d_inner + 2 * d_state + self.nheads, bias=False)
        self.conv1d = nn.Conv1d(conv_dim, conv_dim, d_conv, groups=conv_dim, padding=d_conv - 1, bias=True)
        self.dt_bias = nn.Parameter(torch.zeros(self.nheads))
        self.A_log = nn.Parameter(torch.zeros(self.nheads))
        self.D = nn.Parameter(torch.ones(self.nheads))
        self.norm = nn.Module()
        self.norm.weight = nn.Parameter(torch.ones(self.d_inner))
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=False)

    def forward(self, u):
        p = {k: v.detach().double() for k, v in self.state_dict().items()}
        return mamba2_fp64(p, u.double(), sequential=True).to(u.dtype)


def scan_sequential(x, dt, A, Bm, Cm, Dv):
    """x [B, L, H, P], dt [B, L, H], A [H], Bm / Cm [B, L, N], Dv [H] -> y [B, L, H, P]: the recurrence one token at a time."""
    Bn, L, H, P = x.shape
    S = x.new_zeros(Bn, H, Bm.shape[-1], P)
    y = torch.empty_like(x)
    for t in range(L):
        S = torch.exp(dt[:, t] * A)[:, :, None, None] * S + dt[:, t, :, None, None] * Bm[:, t, None, :, None] * x[:, t, :, None, :]
        y[:, t] = torch.einsum("bn,bhnp->bhp", Cm[:, t], S) + Dv[None, :, None] * x[:, t]
    return y


def scan_chunked(x, dt, A, Bm, Cm, Dv, Q: int = 64):
    """The same scan in chunks of Q tokens, with a_i = dt_i A and s_i = sum_{k<=i} a_k inside a chunk:
        y_i   = sum_{j<=i} exp(s_i - s_j) dt_j (C_i . B_j) x_j + exp(s_i) C_i^T S_in + D x_i
        S_out = exp(s_{Q-1}) S_in + sum_j exp(s_{Q-1} - s_j) dt_j B_j x_j^T
    Only differences <= 0 are exponentiated, and the j > i entries are exactly 0 before any multiply."""
    Bn, L, H, P = x.shape
    S = x.new_zeros(Bn, H, Bm.shape[-1], P)
    y = torch.empty_like(x)
    for c0 in range(0, L, Q):
        c1 = min(c0 + Q, L)
        q = c1 - c0
        xc, dtc, Bc, Cc = x[:, c0:c1], dt[:, c0:c1], Bm[:, c0:c1], Cm[:, c0:c1]
        s = torch.cumsum(dtc * A, dim=1)                                        # [B, q, H]
        tri = torch.tril(torch.ones(q, q, dtype=torch.bool, device=x.device))
        diff = torch.where(tri[None, :, :, None], s[:, :, None, :] - s[:, None, :, :], torch.zeros((), dtype=x.dtype, device=x.device))
        decay = torch.where(tri[None, :, :, None], torch.exp(diff), torch.zeros((), dtype=x.dtype, device=x.device))   # [B, i, j, H]
        G = torch.einsum("bin,bjn->bij", Cc, Bc)[..., None] * decay * dtc[:, None, :, :]
        yc = torch.einsum("bijh,bjhp->bihp", G, xc)
        yc = yc + torch.exp(s)[..., None] * torch.einsum("bin,bhnp->bihp", Cc, S)
        y[:, c0:c1] = yc + Dv[None, None, :, None] * xc
        w = torch.exp(s[:, -1:, :] - s) * dtc                                 # [B, q, H]
        S = torch.exp(s[:, -1])[:, :, None, None] * S + torch.einsum("bjh,bjn,bjhp->bhnp", w, Bc, xc)
    return y


def mamba2_fp64(p: dict, u: torch.Tensor, sequential: bool = False, Q: int = 64) -> torch.Tensor:
    """One Mamba2 layer on u [B, L, d_model] (float64); p: its state_dict (keys without a prefix), float64."""
    Bn, L, _ = u.shape
    H = p["A_log"].shape[0]
    d_inner = p["norm.weight"].shape[0]
    P, N = d_inner // H, (p["conv1d.bias"].shape[0] - d_inner) // 2
    zxbcdt = u @ p["in_proj.weight"].T
    z, xBC, dt = zxbcdt.split([d_inner, d_inner + 2 * N, H], dim=-1)
    xBC = F.conv1d(xBC.transpose(1, 2), p["conv1d.weight"], p["conv1d.bias"], padding=D_CONV - 1, groups=xBC.shape[-1])[..., :L]
    xBC = F.silu(xBC.transpose(1, 2))
    x, Bm, Cm = xBC.split([d_inner, N, N], dim=-1)
    dt = F.softplus(dt + p["dt_bias"])
    A = -torch.exp(p["A_log"])
    scan = scan_sequential if sequential else lambda *a: scan_chunked(*a, Q=Q)
    y = scan(x.reshape(Bn, L, H, P), dt, A, Bm, Cm, p["D"]).reshape(Bn, L, d_inner)
    g = y * F.silu(z)
    g = g * torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + 1e-5) * p["norm.weight"]
    return g @ p["out_proj.weight"].T


def _layer_prefix(variant: str, i: int) -> str:
    return f"mamba_layers.{i}.mamba." if variant == "mamba" else f"mamba_layers.{i}."


def mamba_forward_fp64(variant: str, sd: dict, ids, mask=None, trace: dict | None = None, device=None) -> torch.Tensor:
    """Logits [B, 2] (float64) of the reference net `variant` in eval mode (dropout off); `mask` [B, L] is the second forward
    argument (`mamba` multiplies by it, `mambasp` ignores it).  `trace` receives "front" and "layer0" [B, L, d] and "pooled" [B, d].
    Runs on `device` (default: the CPU)."""
    dev = torch.device(device or "cpu")
    w = {k: v.detach().to(dev, torch.float64) for k, v in sd.items()}
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64, device=dev)
    L = ids.shape[1]
    n_layers = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("mamba_layers."))
    h = F.embedding(ids, w["embedding.weight"])
    if variant == "mamba":
        if L > w["pos_embedding"].shape[1]:
            raise ValueError(f"read length {L} exceeds model_max_length {w['pos_embedding'].shape[1]}")
        h = h + w["pos_embedding"][:, :L]
        h = F.linear(h, w["input_block.0.weight"], w["input_block.0.bias"])
        h = F.layer_norm(h, (h.shape[-1],), w["input_block.1.weight"], w["input_block.1.bias"], eps=1e-5)
        m = None if mask is None else torch.as_tensor(np.asarray(mask), dtype=torch.float64, device=dev)[..., None]
        if m is not None:
            h = h * m
    else:
        m = None
    if trace is not None:
        trace["front"] = h
    for i in range(n_layers):
        pre = _layer_prefix(variant, i)
        p = {k[len(pre):]: v for k, v in w.items() if k.startswith(pre)}
        h = h + mamba2_fp64(p, h)
        if m is not None:
            h = h * m
        if trace is not None and i == 0:
            trace["layer0"] = h
    pooled = (h.mean(1) + h.max(1)[0]) / 2
    if trace is not None:
        trace["pooled"] = pooled
    x = F.gelu(F.linear(pooled, w["pooler.0.weight"], w["pooler.0.bias"]))
    x = F.gelu(F.linear(x, w["classifier.0.weight"], w["classifier.0.bias"]))
    return F.linear(x, w["classifier.3.weight"], w["classifier.3.bias"])


def make_mamba_state_dict(variant: str, seed: int, d_state: int | None = None, n_layers: int | None = None,
                          model_max_length: int | None = None, d_model: int | None = None,
                          expand: int | None = None) -> dict[str, torch.Tensor]:
    """The reference's state_dict layout for `variant` from numpy's default_rng(seed), fp32.  Mamba2 parameters follow mamba_ssm's
    initialisation (A uniform in [1, 16], dt log-uniform in [1e-3, 0.1] through the inverse softplus into dt_bias), with D and
    norm.weight spread around 1 so that both show; projections at 1/sqrt(fan-in); the classifier is scaled and its bias centred on
    seeded calibration reads so that logits are O(1) with both labels present."""
    d, nl, N, expand_, mml = VARIANTS[variant]
    N = d_state or N
    nl = n_layers or nl
    d = d_model or d
    expand = expand or expand_
    mml = model_max_length or mml
    rng = np.random.default_rng(seed)
    di = expand * d
    H = di // HEADDIM
    sd = {"embedding.weight": rng.normal(0.0, 1.0, (VOCAB, d))}
    if variant == "mamba":
        sd["pos_embedding"] = rng.normal(0.0, 0.02, (1, mml, d))
        sd["input_block.0.weight"] = rng.normal(0.0, 1.0 / math.sqrt(d), (d, d))
        sd["input_block.0.bias"] = rng.normal(0.0, 0.1, d)
        sd["input_block.1.weight"] = rng.uniform(0.5, 1.5, d)
        sd["input_block.1.bias"] = rng.normal(0.0, 0.1, d)
    for i in range(nl):
        pre = _layer_prefix(variant, i)
        dt = np.exp(rng.uniform(math.log(1e-3), math.log(0.1), H))
        sd[pre + "dt_bias"] = dt + np.log(-np.expm1(-dt))
        sd[pre + "A_log"] = np.log(rng.uniform(1.0, 16.0, H))
        sd[pre + "D"] = rng.uniform(0.5, 1.5, H)
        sd[pre + "in_proj.weight"] = rng.normal(0.0, 1.0 / math.sqrt(d), (2 * di + 2 * N + H, d))
        sd[pre + "conv1d.weight"] = rng.uniform(-0.5, 0.5, (di + 2 * N, 1, D_CONV))
        sd[pre + "conv1d.bias"] = rng.uniform(-0.5, 0.5, di + 2 * N)
        sd[pre + "norm.weight"] = rng.uniform(0.5, 1.5, di)
        sd[pre + "out_proj.weight"] = rng.normal(0.0, 0.5 / math.sqrt(di), (d, di))
    sd["pooler.0.weight"] = rng.normal(0.0, 1.0 / math.sqrt(d), (d, d))
    sd["pooler.0.bias"] = rng.normal(0.0, 0.1, d)
    sd["classifier.0.weight"] = rng.normal(0.0, 2.0 / math.sqrt(d), (d // 2, d))
    sd["classifier.0.bias"] = rng.normal(0.0, 0.1, d // 2)
    sd["classifier.3.weight"] = rng.normal(0.0, 5.0 / math.sqrt(d // 2), (2, d // 2))
    sd["classifier.3.bias"] = np.zeros(2)
    sd = {k: torch.from_numpy(np.asarray(v)).float() for k, v in sd.items()}
    centre = mamba_forward_fp64(variant, sd, synthetic_ids(seed + 7919, 8, 200)).mean(0)
    sd["classifier.3.bias"] = (torch.from_numpy(rng.normal(0.0, 0.3, 2)) - centre).float()
    return sd


def synthetic_ids(seed: int, batch: int, length: int, pads: int = 0) -> np.ndarray:
    """int64 [B, L]: A/C/G/T (7..10) with a base composition of its own per read, N (11) with p = 0.002, a few other ids of the
    vocabulary, optional left padding with [PAD] = 4."""
    rng = np.random.default_rng(seed)
    ids = np.empty((batch, length), dtype=np.int64)
    for b in range(batch):
        ids[b] = 7 + rng.choice(4, size=length, p=rng.dirichlet(np.full(4, 0.7)))
    ids[rng.random((batch, length)) < 0.002] = 11
    odd = rng.random((batch, length)) < 0.001
    ids[odd] = rng.integers(0, 7, size=int(odd.sum()))
    if pads:
        ids[:, :pads] = PAD
    return ids
