"""The attention pooling of the Hyena head, forward and backward, as closed formulas in torch (dtype as an argument, ln_f included):
what csrc/pool_train.hip computes, for tests/test_headtrain_host.py (held to fp64 autograd of the oracle's head) and
tests/test_gpu_headtrain.py (the kernel's reference, in fp64, and its error yardstick, in float32 on the CPU).

Per read, x_t = ln_f(h_t):  u_t = W1 x_t + b1,  g_t = gelu_erf(u_t),  s_t = w2 . g_t + b2,  a = softmax_t(s),  p = sum_t a_t x_t.
Given dp = dloss/dp:  ds_t = a_t ((x_t - p) . dp),  dw2 = sum ds_t g_t,  db2 = sum ds_t,  du_t = ds_t w2 * gelu'(u_t) with
gelu'(u) = Phi(u) + u phi(u),  db1 = sum du_t,  dW1 = sum_t du_t x_t^T.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def pool_forward(rows, lnf_g, lnf_b, w1, b1, w2, b2, dt=torch.float64):
    """rows [B, L, 256] -> dict(x, u, scores [B, L], attn [B, L], pooled [B, 256]) in dtype `dt`."""
    rows, lnf_g, lnf_b, w1, b1, w2, b2 = (t.to(dt) for t in (rows, lnf_g, lnf_b, w1, b1, w2, b2))
    x = F.layer_norm(rows, (rows.shape[-1],), lnf_g, lnf_b, LN_EPS)
    u = x @ w1.T + b1
    g = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    s = g @ w2.reshape(-1) + b2.reshape(())
    a = torch.softmax(s, dim=1)
    return {"x": x, "u": u, "g": g, "scores": s, "attn": a, "pooled": (a.unsqueeze(-1) * x).sum(dim=1)}


def pool_backward(fwd, w2, dpooled):
    """The formulas: (dW1 [256, 256], db1 [256], dw2 [256], db2 []) from `pool_forward`'s dict and dloss/dpooled [B, 256]."""
    x, u, g, a, p = fwd["x"], fwd["u"], fwd["g"], fwd["attn"], fwd["pooled"]
    dt = x.dtype
    dp, w2 = dpooled.to(dt), w2.to(dt).reshape(-1)
    ds = a * ((x - p.unsqueeze(1)) * dp.unsqueeze(1)).sum(dim=-1)                       # [B, L]
    dw2 = (ds.unsqueeze(-1) * g).sum(dim=(0, 1))
    db2 = ds.sum()
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    du = ds.unsqueeze(-1) * w2 * (cdf + u * pdf)                                        # [B, L, 256]
    db1 = du.sum(dim=(0, 1))
    dw1 = torch.einsum("blf,blc->fc", du, x)
    return dw1, db1, dw2, db2


def pool_grads(rows, lnf_g, lnf_b, w1, b1, w2, b2, dpooled, dt=torch.float64):
    fwd = pool_forward(rows, lnf_g, lnf_b, w1, b1, w2, b2, dt)
    return fwd, pool_backward(fwd, w2, dpooled)


def rel_err(got, want) -> float:
    """max |got - want| / max |want| in fp64 (0 when both are all zero)."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    scale = float(want.abs().max())
    diff = float((got - want).abs().max())
    return diff / scale if scale > 0 else diff


def seeded_case(B: int, L: int, seed: int = 0, w2_scale: float = 1.0, sd=None):
    """Rows (seeded normal x 3 + 0.5), the head's pooling weights of `oracle.make_state_dict` (w2 scaled) and a seeded dpooled."""
    from oracle import hyena_oracle as ho

    sd = sd if sd is not None else ho.make_state_dict(0)
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + L)
    rows = torch.randn(B, L, 256, generator=g) * 3.0 + 0.5
    dpooled = torch.randn(B, 256, generator=g)
    return {"rows": rows, "dpooled": dpooled, "lnf_g": sd[ho.BB + "ln_f.weight"].float(), "lnf_b": sd[ho.BB + "ln_f.bias"].float(),
            "w1": sd[ho.HD + "attention.0.weight"].float().clone(), "b1": sd[ho.HD + "attention.0.bias"].float().clone(),
            "w2": sd[ho.HD + "attention.2.weight"].float().clone() * w2_scale, "b2": sd[ho.HD + "attention.2.bias"].float().clone()}
