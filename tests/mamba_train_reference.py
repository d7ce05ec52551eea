"""The Mamba2 core in training form, stated twice for the tests of chimeralm_amd.mambatrain (csrc/mamba_train.hip):

* `core_forward` -- the forward in torch ops, any dtype, nothing detached: autograd through it is the ground truth;
* `core_backward` -- the hand formulas the HIP kernels implement (the chunked SSD backward with Q = 64, gate + gated RMSNorm,
  softplus, conv + SiLU), also in torch ops and any dtype.  Evaluated in float64 it is the reference of the GPU tests; evaluated in
  float32 on the CPU it gives the error those formulas have in the engine's number format, which sets the tests' bound.

`dA_log`, `d dt_bias` and the `dt` columns of `dzxbcdt` are differences of large sums; `core_backward` returns, next to each of them,
the sum of the absolute terms (`*_abs`): the size of what cancels, which is the denominator of their relative error.  The other
batch-reduced gradients (`conv1d.weight`, `conv1d.bias`, `norm.weight`, `D`) carry theirs too, per channel or head, for the row-wise
comparison (tests/grad_rows.py).  `DEFECTS` are wrong variants of the formulas, planted by tests/test_grad_rows_host.py into the
float32 evaluation only.

`net_forward` is the whole net (either variant) around `core_forward`, differentiable in every parameter, with the max-pool routed by
a given argmax (`route`), so that a near-tie cannot turn a rounding difference into another gradient.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from mamba_reference import D_CONV, PAD, scan_chunked, _layer_prefix

EPS = 1e-5
CORE_PARAMS = ("conv1d.weight", "conv1d.bias", "dt_bias", "A_log", "D", "norm.weight")
# carry_no_decay: dS crosses a chunk boundary without its exp(s_last) | carry_reset: dS of the chunks behind is dropped at every
# boundary but the first one crossed | pad_dt: the last chunk is staged as Q rows and its rows t >= L keep the dt of the rows that
# follow in memory (x, B, C, dy are 0 there) | conv_across_reads: the conv backward's taps reach from the end of read b into read
# b + 1 | no_ub: ddt without its ub term
DEFECTS = ("carry_no_decay", "carry_reset", "pad_dt", "conv_across_reads", "no_ub")


def dims_of(p: dict) -> tuple[int, int, int]:
    """(d_inner, H, N) from a core parameter dict."""
    H = p["A_log"].shape[0]
    di = p["norm.weight"].shape[0]
    return di, H, (p["conv1d.bias"].shape[0] - di) // 2


def dsilu(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


def _pieces(zx, p):
    di, H, N = dims_of(p)
    L = zx.shape[1]
    z, xBC, raw = zx.split([di, di + 2 * N, H], dim=-1)
    u = F.conv1d(xBC.transpose(1, 2), p["conv1d.weight"], p["conv1d.bias"], padding=D_CONV - 1, groups=xBC.shape[-1])[..., :L].transpose(1, 2)
    xc = F.silu(u)
    dt = F.softplus(raw + p["dt_bias"])
    A = -torch.exp(p["A_log"])
    return z, xBC, raw, u, xc, dt, A


def core_forward(zx: torch.Tensor, p: dict, Q: int = 64) -> torch.Tensor:
    """out [B, L, d_inner] of zxbcdt [B, L, 2 di + 2 N + H] under the six core parameters `p` (keys CORE_PARAMS)."""
    di, H, N = dims_of(p)
    Bn, L, _ = zx.shape
    z, _, _, _, xc, dt, A = _pieces(zx, p)
    x, Bm, Cm = xc.split([di, N, N], dim=-1)
    ys = scan_chunked(x.reshape(Bn, L, H, di // H), dt, A, Bm, Cm, p["D"], Q=Q).reshape(Bn, L, di)
    g = ys * F.silu(z)
    return g * torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + EPS) * p["norm.weight"]


def _rcumsum(v, dim):
    return torch.flip(torch.cumsum(torch.flip(v, (dim,)), dim), (dim,))


def scan_backward(x, dt, A, Bm, Cm, Dv, dy, Q: int = 64, defect: str | None = None) -> dict:
    """The chunked backward of `scan_chunked` (y includes D x).  x, dy [B, L, H, P], dt [B, L, H], A, Dv [H], Bm, Cm [B, L, N].
    -> dx, ddt, dA, dB, dC, dD and ddt_abs, dA_abs, dD_abs (sums of the absolute terms)."""
    Bn, L, H, P = x.shape
    zero = torch.zeros((), dtype=x.dtype)
    states, S = [], x.new_zeros(Bn, H, Bm.shape[-1], P)
    for c0 in range(0, L, Q):                                   # the chunks' entry states, as the forward leaves them
        c1 = min(c0 + Q, L)
        states.append(S)
        s = torch.cumsum(dt[:, c0:c1] * A, dim=1)
        w = torch.exp(s[:, -1:] - s) * dt[:, c0:c1]
        S = torch.exp(s[:, -1])[:, :, None, None] * S + torch.einsum("bjh,bjn,bjhp->bhnp", w, Bm[:, c0:c1], x[:, c0:c1])
    dx, ddt, ddt_abs = torch.empty_like(x), torch.empty_like(dt), torch.empty_like(dt)
    dB, dC = torch.empty_like(Bm), torch.empty_like(Cm)
    dA, dA_abs = x.new_zeros(H), x.new_zeros(H)
    dS = torch.zeros_like(S)
    for ci in reversed(range(len(states))):
        c0, c1 = ci * Q, min(ci * Q + Q, L)
        q = c1 - c0
        xc, dtc, Bc, Cc, dyc, Sin = x[:, c0:c1], dt[:, c0:c1], Bm[:, c0:c1], Cm[:, c0:c1], dy[:, c0:c1], states[ci]
        s = torch.cumsum(dtc * A, dim=1)                                                  # [B, q, H]
        tri = torch.tril(torch.ones(q, q, dtype=torch.bool))[None, :, :, None]
        Lm = torch.where(tri, torch.exp(torch.where(tri, s[:, :, None, :] - s[:, None, :, :], zero)), zero)   # [B, i, j, H]
        e, f, e_last = torch.exp(s), torch.exp(s[:, -1:] - s), torch.exp(s[:, -1])
        CB = torch.einsum("bin,bjn->bij", Cc, Bc)[..., None]
        DX = torch.einsum("bihp,bjhp->bijh", dyc, xc)
        dtj = dtc[:, None, :, :]
        G, W, Kl = Lm * dtj * CB, Lm * dtj * DX, Lm * CB * DX
        K = Kl * dtj
        BdS = torch.einsum("bjn,bhnp->bjhp", Bc, dS)
        dx[:, c0:c1] = torch.einsum("bijh,bihp->bjhp", G, dyc) + (f * dtc)[..., None] * BdS + Dv[None, None, :, None] * dyc
        dCi = e[..., None] * torch.einsum("bihp,bhnp->bihn", dyc, Sin)                    # the inter-chunk part of dC, per head
        dC[:, c0:c1] = (torch.einsum("bijh,bjn->bihn", W, Bc) + dCi).sum(2)
        XdS = torch.einsum("bjhp,bhnp->bjhn", xc, dS)
        dB[:, c0:c1] = (torch.einsum("bijh,bin->bjhn", W, Cc) + (f * dtc)[..., None] * XdS).sum(2)
        ub = f * torch.einsum("bjn,bjhn->bjh", Bc, XdS)
        u = ub * dtc
        r = torch.einsum("bin,bihn->bih", Cc, dCi)
        dot = torch.einsum("bhnp,bhnp->bh", dS, Sin)
        ds = K.sum(2) - K.sum(1) + r - u
        ds[:, -1] = ds[:, -1] + u.sum(1) + e_last * dot
        da = _rcumsum(ds, 1)
        ddt[:, c0:c1] = Kl.sum(1) + (0 if defect == "no_ub" else ub) + A * da
        dA = dA + (da * dtc).sum((0, 1))
        ub_a = f * torch.einsum("bjn,bjhn->bjh", Bc.abs(), XdS.abs())
        ds_a = K.abs().sum(2) + K.abs().sum(1) + torch.einsum("bin,bihn->bih", Cc.abs(), dCi.abs()) + ub_a * dtc
        ds_a[:, -1] = ds_a[:, -1] + (ub_a * dtc).sum(1) + e_last * torch.einsum("bhnp,bhnp->bh", dS.abs(), Sin.abs())
        da_a = _rcumsum(ds_a, 1)
        ddt_abs[:, c0:c1] = Kl.abs().sum(1) + ub_a + A.abs() * da_a
        dA_abs = dA_abs + (da_a * dtc).sum((0, 1))
        carried = e_last[:, :, None, None] * dS
        if defect == "carry_no_decay":
            carried = dS
        elif defect == "carry_reset" and ci < len(states) - 1:
            carried = torch.zeros_like(dS)
        dS = carried + torch.einsum("bin,bih,bihp->bhnp", Cc, e, dyc)
    return {"dx": dx, "ddt": ddt, "dA": dA, "dB": dB, "dC": dC, "dD": (dy * x).sum((0, 1, 3)), "ddt_abs": ddt_abs, "dA_abs": dA_abs,
            "dD_abs": (dy * x).abs().sum((0, 1, 3))}


def _scan_backward_padded(x, dt, A, Bm, Cm, Dv, dy, Q: int) -> dict:
    """`scan_backward` with the last chunk staged as Q rows: x, B, C, dy zero past L, dt that of the rows that follow in the flattened
    [B L] rows (read b + 1's first ones; behind the last read, read 0's)."""
    L = x.shape[1]
    n = -L % Q
    zp = lambda t: torch.cat([t, torch.zeros_like(t[:, :n])], dim=1)           # noqa: E731
    sb = scan_backward(zp(x), torch.cat([dt, torch.roll(dt, -1, 0)[:, :n]], dim=1), A, zp(Bm), zp(Cm), Dv, zp(dy), Q=Q)
    return {k: (v[:, :L] if v.dim() > 1 else v) for k, v in sb.items()}


def core_backward(zx: torch.Tensor, p: dict, dout: torch.Tensor, Q: int = 64, defect: str | None = None) -> dict:
    """The hand formulas: -> "out", "dzxbcdt", one entry per CORE_PARAMS key, "dzxbcdt_dt_abs" and "<key>_abs" for every CORE_PARAMS
    key.  `defect`: one of DEFECTS, planted."""
    di, H, N = dims_of(p)
    Bn, L, _ = zx.shape
    P = di // H
    z, xBC, raw, u, xc, dt, A = _pieces(zx, p)
    x, Bm, Cm = xc.split([di, N, N], dim=-1)
    ys = scan_chunked(x.reshape(Bn, L, H, P), dt, A, Bm, Cm, p["D"], Q=Q).reshape(Bn, L, di)
    sz, w = F.silu(z), p["norm.weight"]
    g = ys * sz
    r = torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + EPS)
    out = g * r * w
    dg = r * w * dout - g * r ** 3 * (g * w * dout).mean(-1, keepdim=True)
    dys, dz = dg * sz, dg * ys * dsilu(z)
    if defect == "pad_dt":
        sb = _scan_backward_padded(x.reshape(Bn, L, H, P), dt, A, Bm, Cm, p["D"], dys.reshape(Bn, L, H, P), Q)
    else:
        sb = scan_backward(x.reshape(Bn, L, H, P), dt, A, Bm, Cm, p["D"], dys.reshape(Bn, L, H, P), Q=Q, defect=defect)
    sg = torch.sigmoid(raw + p["dt_bias"])
    draw, draw_abs = sb["ddt"] * sg, sb["ddt_abs"] * sg
    du = torch.cat([sb["dx"].reshape(Bn, L, di), sb["dB"], sb["dC"]], dim=-1) * dsilu(u)
    xpad = F.pad(xBC, (0, 0, D_CONV - 1, 0))                                             # [B, L + 3, conv_dim]
    dupad = F.pad(du, (0, 0, 0, D_CONV - 1))
    if defect == "conv_across_reads":
        dupad[:-1, L:] = du[1:, :D_CONV - 1]
    cw = p["conv1d.weight"][:, 0, :]                                                      # [conv_dim, 4]
    dcw = torch.stack([(du * xpad[:, k:k + L]).sum((0, 1)) for k in range(D_CONV)], dim=-1)
    dcw_abs = torch.stack([(du * xpad[:, k:k + L]).abs().sum((0, 1)) for k in range(D_CONV)], dim=-1)
    dxBC = sum(cw[:, k] * dupad[:, D_CONV - 1 - k:D_CONV - 1 - k + L] for k in range(D_CONV))
    return {"out": out, "dzxbcdt": torch.cat([dz, dxBC, draw], dim=-1), "conv1d.weight": dcw[:, None, :], "conv1d.bias": du.sum((0, 1)),
            "dt_bias": draw.sum((0, 1)), "A_log": A * sb["dA"], "D": sb["dD"], "norm.weight": (dout * g * r).sum((0, 1)),
            "A_log_abs": A.abs() * sb["dA_abs"], "dt_bias_abs": draw_abs.sum((0, 1)), "dzxbcdt_dt_abs": draw_abs,
            "conv1d.weight_abs": dcw_abs[:, None, :], "conv1d.bias_abs": du.abs().sum((0, 1)), "D_abs": sb["dD_abs"],
            "norm.weight_abs": (dout * g * r).abs().sum((0, 1))}


def autograd_core(zx: torch.Tensor, p: dict, dout: torch.Tensor, sequential: bool = False) -> dict:
    """The same quantities from torch autograd through `core_forward` (or, `sequential`, through `scan_sequential`)."""
    from mamba_reference import scan_sequential

    zx = zx.detach().clone().requires_grad_(True)
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    if sequential:
        di, H, N = dims_of(q)
        Bn, L, _ = zx.shape
        z, _, _, _, xc, dt, A = _pieces(zx, q)
        x, Bm, Cm = xc.split([di, N, N], dim=-1)
        ys = scan_sequential(x.reshape(Bn, L, H, di // H), dt, A, Bm, Cm, q["D"]).reshape(Bn, L, di)
        g = ys * F.silu(z)
        out = g * torch.rsqrt(g.pow(2).mean(-1, keepdim=True) + EPS) * q["norm.weight"]
    else:
        out = core_forward(zx, q)
    grads = torch.autograd.grad(out, [zx] + [q[k] for k in CORE_PARAMS], dout)
    res = {"out": out.detach(), "dzxbcdt": grads[0]}
    res.update({k: gr for k, gr in zip(CORE_PARAMS, grads[1:])})
    return res


def random_core(seed: int, d_model: int, expand: int, N: int, Bn: int, L: int, dt_range=None, A_value=None, dtype=torch.float64):
    """Seeded (zxbcdt, params, dout) of a core; `dt_range` = (lo, hi) makes softplus(raw + dt_bias) uniform in it, `A_value` fixes A."""
    g = torch.Generator().manual_seed(seed)
    di = expand * d_model
    H, cd = di // 64, di + 2 * N
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    uni = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float64)   # noqa: E731
    zx = rnd(Bn, L, 2 * di + 2 * N + H)
    dt0 = torch.exp(uni(-6.9, -2.3, H))
    p = {"conv1d.weight": uni(-0.5, 0.5, cd, 1, D_CONV), "conv1d.bias": uni(-0.5, 0.5, cd), "dt_bias": dt0 + torch.log(-torch.expm1(-dt0)),
         "A_log": torch.log(uni(1.0, 16.0, H)), "D": uni(0.5, 1.5, H), "norm.weight": uni(0.5, 1.5, di)}
    if dt_range is not None:
        want = uni(dt_range[0], dt_range[1], Bn, L, H)
        zx[..., 2 * di + 2 * N:] = want + torch.log(-torch.expm1(-want)) - p["dt_bias"]      # the inverse softplus
    if A_value is not None:
        p["A_log"] = torch.full((H,), float(A_value), dtype=torch.float64).log()
    dout = rnd(Bn, L, di)
    return zx.to(dtype), {k: v.to(dtype) for k, v in p.items()}, dout.to(dtype)


# ------------------------------------------------------------------------------------------------------------- the whole net
def net_forward(variant: str, w: dict, ids: torch.Tensor, mask: torch.Tensor | None = None, route: torch.Tensor | None = None,
                taps: list | None = None):
    """(logits [B, 2], pooled [B, d], argmax of the max-pool [B, d]) of the reference net in training mode at dropout 0, in the dtype
    of `w` (its state_dict as tensors, possibly requiring grad).  `route` [B, d]: the positions the max-pool takes.  `taps` receives
    every layer's (zxbcdt, core output), the output keeping its gradient."""
    L = ids.shape[1]
    n_layers = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("mamba_layers."))
    h = F.embedding(ids, w["embedding.weight"], padding_idx=PAD)
    m = None
    if variant == "mamba":
        h = h + w["pos_embedding"][:, :L]
        h = F.linear(h, w["input_block.0.weight"], w["input_block.0.bias"])
        h = F.layer_norm(h, (h.shape[-1],), w["input_block.1.weight"], w["input_block.1.bias"], eps=1e-5)
        if mask is not None:
            m = mask.to(h.dtype)[..., None]
            h = h * m
    for i in range(n_layers):
        pre = _layer_prefix(variant, i)
        p = {k: w[pre + k] for k in CORE_PARAMS}
        zx = F.linear(h, w[pre + "in_proj.weight"])
        y = core_forward(zx, p)
        if taps is not None:
            y.retain_grad()
            taps.append((zx, y))
        h = h + F.linear(y, w[pre + "out_proj.weight"])
        if m is not None:
            h = h * m
    arg = h.argmax(1) if route is None else route
    pooled = (h.mean(1) + h.gather(1, arg[:, None, :])[:, 0]) / 2
    x = F.gelu(F.linear(pooled, w["pooler.0.weight"], w["pooler.0.bias"]))
    x = F.gelu(F.linear(x, w["classifier.0.weight"], w["classifier.0.bias"]))
    return F.linear(x, w["classifier.3.weight"], w["classifier.3.bias"]), pooled, arg


def net_step(variant: str, sd: dict, ids, labels, mask=None, route=None, dtype=torch.float64) -> dict:
    """One training step's loss, logits, pooled and the gradient of every parameter, in `dtype` on the CPU; "den": for every
    `A_log` and `dt_bias` key the sum of the absolute terms of its gradient (`core_backward` on the layer's own input and `dout`)."""
    w = {k: v.detach().to("cpu", dtype).requires_grad_(True) for k, v in sd.items()}
    ids = torch.as_tensor(ids, dtype=torch.int64).cpu()
    mask = None if mask is None else torch.as_tensor(mask).cpu()
    taps: list = []
    logits, pooled, arg = net_forward(variant, w, ids, mask, None if route is None else torch.as_tensor(route).cpu(), taps)
    loss = F.cross_entropy(logits, torch.as_tensor(labels, dtype=torch.int64).cpu())
    loss.backward()
    den = {}
    with torch.no_grad():
        for i, (zx, y) in enumerate(taps):
            pre = _layer_prefix(variant, i)
            cb = core_backward(zx.detach(), {k: w[pre + k].detach() for k in CORE_PARAMS}, y.grad)
            den[pre + "A_log"], den[pre + "dt_bias"] = cb["A_log_abs"], cb["dt_bias_abs"]
    return {"den": den, "loss": loss.detach(), "logits": logits.detach(), "pooled": pooled.detach(), "route": arg,
            "grads": {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}}
