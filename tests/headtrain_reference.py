"""The attention pooling of the Hyena head, forward and backward, as closed formulas in torch (dtype as an argument, ln_f included):
what csrc/pool_train.hip computes, for tests/test_headtrain_host.py (held to fp64 autograd of the oracle's head) and
tests/test_gpu_headtrain.py (the kernel's reference, in fp64, and its error yardstick, in float32 on the CPU); tests/grad_rows.py cuts
the same outputs into rows, each over its own sum of absolute terms, which the two functions return beside the values.

Per read, x_t = ln_f(h_t):  u_t = W1 x_t + b1,  g_t = u_t Phi(u_t) (Phi = 0.5 erfc(-u / sqrt 2): `cdf`),  s_t = w2 . g_t + b2,  a = softmax_t(s),  p = sum_t a_t x_t.
Given dp = dloss/dp:  ds_t = a_t ((x_t - p) . dp),  dw2 = sum ds_t g_t,  db2 = sum ds_t,  du_t = ds_t w2 * gelu'(u_t) with
gelu'(u) = Phi(u) + u phi(u),  db1 = sum du_t,  dW1 = sum_t du_t x_t^T.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


DEFECTS = ("cdf_erf", "last_tile", "no_p", "no_updf", "stats0", "w2_missing", "x_nobias", "stale_read")
TILE = 64                                      # csrc/mfma32_common.h BM32: the backward's token tile


def cdf(u):
    """The normal cdf as 0.5 erfc(-u / sqrt 2), in every dtype: 0.5 (1 + erf) is a multiple of 2^-25 in float32 and of 2^-54 in float64,
    so below u = -5.4 a float32 evaluation holds 0 or a few quanta next to a true 1e-8 (and float64 itself is off by 6e-4 at u = -8)."""
    return 0.5 * torch.special.erfc(u * -(1.0 / math.sqrt(2.0)))


def _tsum(v, reverse):
    """Sum over the leading (token) dimension; `reverse`: the same terms in mirrored order (the second evaluation)."""
    return (v.flip(0) if reverse else v).sum(0)


def pool_forward(rows, lnf_g, lnf_b, w1, b1, w2, b2, dt=torch.float64, reverse=False):
    """rows [B, L, 256] -> dict(x, u, g, scores [B, L], stats [B, 2] = (max, sum), attn [B, L], pooled [B, 256]) in dtype `dt`, the
    weights the backward needs, and the sums of absolute terms `scores_abs` [B, L], `pooled_abs` [B, 256]."""
    rows, lnf_g, lnf_b, w1, b1, w2, b2 = (t.to(dt) for t in (rows, lnf_g, lnf_b, w1, b1, w2, b2))
    w2 = w2.reshape(-1)
    x = F.layer_norm(rows, (rows.shape[-1],), lnf_g, lnf_b, LN_EPS)
    u = x @ w1.T + b1
    g = u * cdf(u)
    s = g @ w2 + b2.reshape(())
    mx = s.amax(dim=1)
    e = torch.exp(s - mx[:, None])
    sm = _tsum(e.T, reverse)
    a = e / sm[:, None]
    ax = a.unsqueeze(-1) * x
    return {"x": x, "u": u, "g": g, "scores": s, "stats": torch.stack([mx, sm], dim=1), "attn": a,
            "pooled": _tsum(ax.transpose(0, 1), reverse), "lnf_b": lnf_b, "w1": w1, "b1": b1,
            "scores_abs": g.abs() @ w2.abs() + b2.abs().reshape(()), "pooled_abs": ax.abs().sum(dim=1)}


def attn_from(scores, stats):
    """a_t = exp(s_t - max) / sum, in the dtype of `scores`: what pool_bwd_kernel takes from the forward's scores and statistics."""
    return torch.exp(scores - stats[:, :1]) * (1.0 / stats[:, 1:])


def pool_backward(fwd, w2, dpooled, defect=None, reverse=False):
    """The formulas: (dW1 [256, 256], db1 [256], dw2 [256], db2 []) from `pool_forward`'s dict and dloss/dpooled [B, 256].  The sums
    of absolute terms of the four land in fwd["den"].  `defect`: one of DEFECTS, planted by tests/test_headtrain_rows_host.py."""
    assert defect is None or defect in DEFECTS
    x, u, g, a, p = fwd["x"], fwd["u"], fwd["g"], fwd["attn"], fwd["pooled"]
    dt = x.dtype
    B, L, C = x.shape
    dp, w2 = dpooled.to(dt), w2.to(dt).reshape(-1)
    if defect == "x_nobias":                                 # the tile taken before ln_f's bias: u, g and dW1's operand follow it
        x = x - fwd["lnf_b"]
        u = x @ fwd["w1"].T + fwd["b1"]
        g = u * cdf(u)
    if defect == "stats0":                                   # read 0's (max, sum) for every read
        a = attn_from(fwd["scores"], fwd["stats"][:1].expand(B, 2))
    if defect == "stale_read":                               # the last read's tile on read 0's pooled and dpooled
        p, dp = p.clone(), dp.clone()
        p[B - 1], dp[B - 1] = p[0], dp[0]
    xc = x if defect == "no_p" else x - p.unsqueeze(1)
    ds = a * (xc * dp.unsqueeze(1)).sum(dim=-1)                                         # [B, L]
    if defect == "last_tile":
        ds = ds.clone()
        ds[:, (L - 1) // TILE * TILE:] = 0
    c = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) if defect == "cdf_erf" else cdf(u)
    if defect == "cdf_erf":
        g = u * c
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    wf = w2
    if defect == "w2_missing":
        wf = w2.clone()
        wf[12::13] = 1.0
    du = ds.unsqueeze(-1) * wf * (c if defect == "no_updf" else c + u * pdf)            # [B, L, 256]
    dsg = (ds.unsqueeze(-1) * g).reshape(B * L, C)
    du2, x2 = du.reshape(B * L, C), x.reshape(B * L, C)
    dw2 = _tsum(dsg, reverse)
    db2 = _tsum(ds.reshape(B * L), reverse)
    db1 = _tsum(du2, reverse)
    dw1 = du2.flip(0).T @ x2.flip(0) if reverse else du2.T @ x2
    fwd["den"] = {"dW1": du2.abs().T @ x2.abs(), "db1": du2.abs().sum(0), "dw2": dsg.abs().sum(0), "db2": ds.abs().sum()}
    return dw1, db1, dw2, db2


def pool_grads(rows, lnf_g, lnf_b, w1, b1, w2, b2, dpooled, dt=torch.float64, defect=None, reverse=False):
    fwd = pool_forward(rows, lnf_g, lnf_b, w1, b1, w2, b2, dt, reverse)
    return fwd, pool_backward(fwd, w2, dpooled, defect, reverse)


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
