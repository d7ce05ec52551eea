"""DNAConvNet in training mode, restated in torch on the CPU (float64 or float32): the arithmetic the engine's training kernels
(csrc/cnn_train.hip) are held to.  Written from the reference's module structure (cnn.py in `train()`); pinned to the reference class
itself by tests/golden/cnn_train_golden.npz (tests/golden/make_cnn_train_golden.py, tests/test_cnn_train_host.py).

Rows are token-major [B, L_i, 256] wherever they are returned, as the engine's buffers are.  Per block: z = conv "same" on all L_i
positions (block 0 as seven table lookups, so that identical inputs give identical bits); mu, v = mean and BIASED variance over all B L_i positions (those no pooling window covers included); xh = (z - mu) /
sqrt(v + 1e-5); y = gelu_erf(g xh + beta); p = the max over windows of 4, routed by `choice` (given: the engine's, so that a near-tie
decided the other way in fp32 does not count as an error; None: torch's own first maximum); o = p keep / (1 - p_drop).  Then the mean
over positions, fc = Linear, BatchNorm1d on batch statistics, GELU, mask, Linear, and the mean cross-entropy.  The gradients come from
autograd over exactly these formulas; `dz` is the gradient that reaches each block's convolution output.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

K, EPS, MOMENTUM = 7, 1e-5, 0.1
PARAM_KEYS = (["embedding.weight"] + [f"conv_blocks.{i}.{s}" for i in range(3) for s in ("0.weight", "0.bias", "1.weight", "1.bias")] +
              ["fc.0.weight", "fc.0.bias", "fc.1.weight", "fc.1.bias", "fc.4.weight", "fc.4.bias"])


def synthetic_labels(seed: int, batch: int) -> np.ndarray:
    return ((np.arange(batch) + seed) % 2).astype(np.int64)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _bn_train(x, g, b, dims):
    """(normalised x, xh, mean, biased variance) over `dims`; channel axis 1."""
    mu = x.mean(dim=dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=dims, keepdim=True)
    xh = (x - mu) / torch.sqrt(var + EPS)
    shape = [1, -1] + [1] * (x.dim() - 2)
    return g.view(shape) * xh + b.view(shape), mu.flatten(), var.flatten()


def cnn_train_reference(sd: dict, ids, labels, dtype=torch.float64, choice=None, keep=None, fc_keep=None, p_drop: float = 0.0) -> dict:
    """One training step's numbers.  sd: the state_dict before the step; choice: None or three uint8 [B, L_{i+1}, 256]; keep: None or
    three {0, 1} masks [B, L_{i+1}, 256] and fc_keep [B, 512], with p_drop the probability they were drawn at.

    Returns loss, logits, pooled, dpooled, fc0_bias_terms [512] (see below), grads {key: tensor}, z / y / dz / choice (lists of three, token-major), mean / var (lists of three,
    biased), fc_mean / fc_var, running {key: tensor} = every BatchNorm buffer after the step."""
    w = {k: (v.detach().cpu().to(dtype).clone().requires_grad_(True) if k in PARAM_KEYS else v.detach().cpu().clone()) for k, v in sd.items()}
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    scale = 1.0 / (1.0 - p_drop)
    B = ids.shape[0]
    L = ids.shape[1]
    x = None
    zs, ys, chs, means, vars_, counts = [], [], [], [], [], []
    for i in range(3):
        p = f"conv_blocks.{i}."
        if i == 0:
            # block 0 through the table T[dk][tok] = W_0[:, :, dk] . E[tok], as the issue writes it: z_0[b, t] = b_0 + sum_dk T[dk][ids[b,
            # t + dk - 3]], the taps added in order and a position outside the read adding nothing.  Positions with identical inputs then
            # get identical values bit for bit, which a library convolution does not promise (measured: its fp64 left [a - 3e-15, a, a,
            # a] for four identical positions at the end of a read), and the pooling choice on exact ties rests on it.  Row 4
            # (padding_idx) is used in the forward and gets no gradient, as nn.Embedding has it.
            E = w["embedding.weight"]
            pad_row = torch.zeros(E.shape[0], 1, dtype=torch.bool)
            pad_row[4] = True
            table = torch.einsum("oik,ti->kto", w[p + "0.weight"], torch.where(pad_row, E.detach(), E))     # [7, 12, 256]
            table = torch.cat([table, torch.zeros(K, 1, table.shape[2], dtype=dtype)], dim=1)               # row 12: outside the read
            padded = F.pad(ids, (K // 2, K // 2), value=E.shape[0])
            z = w[p + "0.bias"].view(1, 1, -1).expand(B, L, -1)
            for dk in range(K):
                z = z + table[dk][padded[:, dk:dk + L]]
            z = z.transpose(1, 2)                                                                           # [B, 256, L]
        else:
            z = F.conv1d(x, w[p + "0.weight"], w[p + "0.bias"], padding=K // 2)
        z.retain_grad()
        u, mu, var = _bn_train(z, w[p + "1.weight"], w[p + "1.bias"], (0, 2))
        y = _gelu(u)
        Lin, Lout = y.shape[2], y.shape[2] // 4
        win = y[:, :, :4 * Lout].reshape(B, 256, Lout, 4)
        if choice is None:
            ch = F.max_pool1d(y.detach(), 4, return_indices=True)[1] % 4             # torch's own first maximum
        else:
            ch = torch.as_tensor(np.asarray(choice[i]), dtype=torch.int64).transpose(1, 2)
        pooled = win.gather(3, ch.unsqueeze(3)).squeeze(3)
        if keep is not None:
            pooled = pooled * torch.as_tensor(np.asarray(keep[i])).to(dtype).transpose(1, 2) * scale
        zs.append(z); ys.append(y); chs.append(ch); means.append(mu); vars_.append(var); counts.append(B * Lin)
        x = pooled
    pooled = x.mean(dim=2)
    pooled.retain_grad()
    h = F.linear(pooled, w["fc.0.weight"], w["fc.0.bias"])
    h.retain_grad()
    h0 = h
    u, fmu, fvar = _bn_train(h, w["fc.1.weight"], w["fc.1.bias"], (0,))
    u.retain_grad()
    u1 = u
    h = _gelu(u)
    if fc_keep is not None:
        h = h * torch.as_tensor(np.asarray(fc_keep)).to(dtype) * scale
    logits = F.linear(h, w["fc.4.weight"], w["fc.4.bias"])
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    # d fc.0.bias is a sum that cancels to 0 (fc.1 is a BatchNorm): per channel, the sum of the absolute values of every term of it,
    # |g| rstd sum_b (|dy| + |mean dy| + |xh mean(dy xh)|) -- the scale its rounding error is measured against
    with torch.no_grad():
        dy, rstd = u1.grad, 1.0 / torch.sqrt(fvar + EPS)
        xh = (h0 - fmu) * rstd
        fc0_bias_terms = w["fc.1.weight"].abs() * rstd * (dy.abs() + dy.mean(0).abs() + (xh * (dy * xh).mean(0)).abs()).sum(0)
    running = {}
    for prefix, mu, var, n in [(f"conv_blocks.{i}.1.", means[i], vars_[i], counts[i]) for i in range(3)] + [("fc.1.", fmu, fvar, B)]:
        running[prefix + "running_mean"] = (1 - MOMENTUM) * w[prefix + "running_mean"].to(dtype) + MOMENTUM * mu.detach()
        running[prefix + "running_var"] = (1 - MOMENTUM) * w[prefix + "running_var"].to(dtype) + MOMENTUM * var.detach() * n / (n - 1)
        running[prefix + "num_batches_tracked"] = w[prefix + "num_batches_tracked"] + 1
    tm = lambda t: t.detach().transpose(1, 2).contiguous()      # noqa: E731 - [B, C, L] -> token-major
    return {"loss": loss.detach(), "logits": logits.detach(), "pooled": pooled.detach(), "dpooled": pooled.grad.detach(), "fc0_bias_terms": fc0_bias_terms.detach(),
            "grads": {k: w[k].grad.detach() for k in PARAM_KEYS},
            "z": [tm(z) for z in zs], "y": [tm(y) for y in ys], "dz": [tm(z.grad) for z in zs],
            "choice": [c.transpose(1, 2).contiguous().to(torch.uint8) for c in chs],
            "mean": [m.detach() for m in means], "var": [v.detach() for v in vars_], "fc_mean": fmu.detach(), "fc_var": fvar.detach(),
            "running": running}
