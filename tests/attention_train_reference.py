"""CPU reference of the training attention op (csrc/attention_train.hip, `clm_attn_train_*`): the forward with an explicit keep mask,
the log-sum-exp, dq / dk / dv by the op's formulas -- in any dtype, fp64 as the truth and float32 as the yardstick of the bound --
the numpy restatement of the keep mask's `bits`, and the score patterns the GPU tests run.

    s_ij = q_i . k_j / sqrt(32)        lse_i = ln sum_j exp(s_ij)   (natural units here; the op stores lse / ln 2)
    p_ij = exp(s_ij - lse_i)           O_i = sum_j keep_ij p_ij v_j / (1 - p)
    delta_i = sum_d dO_id O_id         dP_ij = dO_i . v_j           dS_ij = p_ij (keep_ij dP_ij / (1 - p) - delta_i)
    dQ_i = sum_j dS_ij k_j / sqrt(32)  dK_j = sum_i dS_ij q_i / sqrt(32)      dV_j = sum_i keep_ij p_ij dO_i / (1 - p)

dS = p (dP - delta) cancels, so a row of dq, dk or dv can be far smaller than its terms.  `backward` returns, next to each of them,
the row's sum of the absolute terms per (read, head, position) -- `dq_abs`, `dk_abs`, `dv_abs` [B, 8, L], the largest of the 32
components -- the denominator of the row-wise comparison (tests/grad_rows.py):
    |dP|_ij = |dO_i| . |v_j|     |delta|_i = sum_d |dO_id| |O_id|     T_ij = p_ij (keep_ij |dP|_ij / (1 - p) + |delta|_i)
    dq_abs_i = max_d sum_j T_ij |k_jd| / sqrt(32)    dk_abs_j = max_d sum_i T_ij |q_id| / sqrt(32)
    dv_abs_j = max_d sum_i keep_ij p_ij |dO_id| / (1 - p)
`DEFECTS` are wrong variants of the formulas, planted by tests/test_grad_rows_host.py into the float32 evaluation only.
"""
from __future__ import annotations

import math

import numpy as np
import torch

HD, NH, D = 32, 8, 256
PATTERNS = ("normal", "large", "flat", "first_tile_max", "ragged_max")
# delta_unscaled: delta_i = sum_j p_ij dP_ij, without keep / (1 - p) | phantom_key: one more key behind the last, s = 0 instead of
# masked (k = v = 0), in the softmax's sum | skip_last_query_tile: the dk | dv pass leaves out the last (ragged) tile of 64 queries
DEFECTS = ("delta_unscaled", "phantom_key", "skip_last_query_tile")


# ------------------------------------------------------------------------------------------------------------- the keep mask
def mix32(x: np.ndarray) -> np.ndarray:
    """The op's 32-bit avalanche mixer on uint32 arrays (arithmetic modulo 2^32)."""
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def bits(seed: int, bh, i, j) -> np.ndarray:
    """bits(seed, b * 8 + h, i, j) of include/chimeralm_hip.h; bh, i, j broadcast."""
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    bh, i, j = (np.asarray(a).astype(np.uint32) for a in (bh, i, j))
    with np.errstate(over="ignore"):
        r = mix32(lo ^ (i * np.uint32(0x9E3779B1)))
        return mix32((r ^ (hi + bh * np.uint32(0x85EBCA77))) + j * np.uint32(0xC2B2AE3D))


def threshold(p: float) -> int:
    """round(p * 2^32) of the float32 the ABI takes."""
    return int(math.floor(float(np.float32(p)) * 2.0 ** 32 + 0.5))


def keep_mask(seed: int, B: int, L: int, p: float, b0: int = 0) -> np.ndarray:
    """keep [B, 8, L, L] bool of reads b0 .. b0 + B - 1."""
    bh = (8 * b0 + np.arange(8 * B)).reshape(B, NH, 1, 1)
    i, j = np.arange(L).reshape(1, 1, L, 1), np.arange(L).reshape(1, 1, 1, L)
    return bits(seed, bh, i, j).astype(np.uint64) >= np.uint64(threshold(p))


# ------------------------------------------------------------------------------------------------------------- the formulas
def heads(x: torch.Tensor) -> torch.Tensor:
    """[B, L, 256] -> [B, 8, L, 32]."""
    B, L, _ = x.shape
    return x.reshape(B, L, NH, HD).permute(0, 2, 1, 3)


def merge(x: torch.Tensor) -> torch.Tensor:
    """[B, 8, L, 32] -> [B, L, 256]."""
    B, _, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, D)


def rscale(p: float, dt) -> torch.Tensor:
    """1 / (1 - p) of the float32 p the ABI takes, evaluated in dt."""
    one = torch.tensor(1.0, dtype=dt)
    return one / (one - torch.tensor(p, dtype=torch.float32).to(dt))


def _with_zero_key(s: torch.Tensor) -> torch.Tensor:
    """The scores with one more key of score 0 behind the last."""
    return torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)


def forward(qkv: torch.Tensor, keep: torch.Tensor | None, p: float, defect: str | None = None):
    """-> out [B, L, 256], lse [B, 8, L] (natural units), P [B, 8, L, L], in qkv's dtype.  keep: [B, 8, L, L] bool or None."""
    dt = qkv.dtype
    q, k, v = (heads(qkv[..., o: o + D]) for o in (0, D, 2 * D))
    s = (q @ k.transpose(-1, -2)) * torch.tensor(1.0 / math.sqrt(HD), dtype=dt)
    lse = torch.logsumexp(_with_zero_key(s) if defect == "phantom_key" else s, dim=-1)
    P = torch.exp(s - lse[..., None])
    Pd = P if keep is None else P * (keep.to(dt) * rscale(p, dt))
    return merge(Pd @ v), lse, P


def backward(qkv: torch.Tensor, keep: torch.Tensor | None, p: float, dout: torch.Tensor, defect: str | None = None):
    """-> dict out, lse, dq, dk, dv ([B, L, 256] each but lse) by the hand formulas, in qkv's dtype, and dq_abs, dk_abs, dv_abs
    [B, 8, L], the rows' sums of the absolute terms.  `defect`: one of DEFECTS, planted."""
    dt = qkv.dtype
    q, k, v = (heads(qkv[..., o: o + D]) for o in (0, D, 2 * D))
    out, lse, P = forward(qkv, keep, p, defect)
    g = heads(dout)
    scale = torch.tensor(1.0, dtype=dt) if keep is None else keep.to(dt) * rscale(p, dt)
    dP = g @ v.transpose(-1, -2)
    delta = (P * dP).sum(dim=-1, keepdim=True) if defect == "delta_unscaled" else (g * heads(out)).sum(dim=-1, keepdim=True)
    dS = P * (scale * dP - delta)
    c = torch.tensor(1.0 / math.sqrt(HD), dtype=dt)
    T = P * (scale * (g.abs() @ v.abs().transpose(-1, -2)) + (g.abs() * heads(out).abs()).sum(dim=-1, keepdim=True))
    dSt, Pt = dS.transpose(-1, -2), (P * scale).transpose(-1, -2)
    if defect == "skip_last_query_tile":
        L = qkv.shape[1]
        dSt, Pt = dSt.clone(), Pt.clone()
        dSt[..., (L - 1) // 64 * 64:] = 0
        Pt[..., (L - 1) // 64 * 64:] = 0
    return {"out": out, "lse": lse, "dq": merge(dS @ k) * c, "dk": merge(dSt @ q) * c, "dv": merge(Pt @ g),
            "dq_abs": ((T @ k.abs()) * c).amax(-1), "dk_abs": ((T.transpose(-1, -2) @ q.abs()) * c).amax(-1),
            "dv_abs": ((P * scale).transpose(-1, -2) @ g.abs()).amax(-1)}


def autograd(qkv: torch.Tensor, keep: torch.Tensor | None, p: float, dout: torch.Tensor):
    """The same through autograd: softmax -> mask / (1 - p) -> @ v."""
    x = qkv.clone().requires_grad_(True)
    q, k, v = (heads(x[..., o: o + D]) for o in (0, D, 2 * D))
    w = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(HD), dim=-1)
    if keep is not None:
        w = w * keep.to(x.dtype) / (1.0 - float(np.float32(p)))
    out = merge(w @ v)
    out.backward(dout)
    return {"out": out.detach(), "dq": x.grad[..., :D], "dk": x.grad[..., D: 2 * D], "dv": x.grad[..., 2 * D:]}


# ------------------------------------------------------------------------------------------------------------- the inputs
def make_qkv(B: int, L: int, pattern: str, seed: int = 0) -> torch.Tensor:
    """fp32 [B, L, 768] whose scores s = q . k / sqrt(32) follow `pattern`; v unit-normal throughout.
    normal: unit-normal q, k | large: |q| |k| / sqrt(32) = 100, peaked rows, lse >> 1 | flat: q = 0, every p = 1 / L |
    first_tile_max: the maximum among the first 64 keys, every later key >= 40 below | ragged_max: the last key (in the last, ragged
    key tile) ~10 above all others."""
    rng = np.random.default_rng(100003 * seed + 1000 * L + 10 * B + PATTERNS.index(pattern))
    x = rng.standard_normal((B, L, 3 * D)).astype(np.float32)
    q, k = x[..., :D].reshape(B, L, NH, HD), x[..., D: 2 * D].reshape(B, L, NH, HD)
    u = np.zeros(HD, np.float32)
    u[0] = 1.0
    if pattern == "large":
        q[:] = q / np.linalg.norm(q, axis=-1, keepdims=True) * np.sqrt(100.0 * np.sqrt(32.0))
        k[:] = k / np.linalg.norm(k, axis=-1, keepdims=True) * np.sqrt(100.0 * np.sqrt(32.0))
    elif pattern == "flat":
        q[:] = 0.0
    elif pattern == "first_tile_max":
        q[:] = 0.05 * q + u * np.sqrt(32.0)
        k[:] = 0.05 * k
        k[..., 0] = -45.0
        k[:, : min(L, 64), :, 0] = rng.uniform(-2.0, 2.0, (B, min(L, 64), NH))
    elif pattern == "ragged_max":
        d = rng.standard_normal((B, 1, NH, HD)).astype(np.float32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        q[:] = 0.3 * q + 2.0 * d
        k[:, L - 1] = 5.0 * np.sqrt(32.0) * d[:, 0]
    return torch.from_numpy(x)


def make_dout(B: int, L: int, seed: int = 0) -> torch.Tensor:
    rng = np.random.default_rng(77 + 100003 * seed + 1000 * L + B)
    return torch.from_numpy(rng.standard_normal((B, L, D)).astype(np.float32))
