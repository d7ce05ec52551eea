"""Reference arithmetic for the segmented Hyena training core (csrc/hyena_longtrain.hip).  TEST INFRASTRUCTURE.

* `segmented_core`: the operator of tests/hyena_train_reference.py as a uniformly partitioned convolution over segments of P tokens
  with overlap-save transforms of N = 2 P points -- the formulas the kernels run, in torch, any dtype and any P.  Same keys as
  `hyena_train_reference.fft_core`.
* `workspace_bytes`: the formula of include/chimeralm_hip.h.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import hyena_train_reference as R

P_ENGINE = 8192
MAX_TOKENS = 4 * P_ENGINE + 1


def segments(L: int, P: int = P_ENGINE) -> int:
    return (L + P - 1) // P


def workspace_bytes(B: int, L: int) -> int:
    """The formula of include/chimeralm_hip.h: twiddles, S filter spectra per channel, two spectra per (read, channel, segment), the
    per-read dk rows, the per-read parameter partials."""
    S, H = segments(L), P_ENGINE + 1
    return (4 * (2 * P_ENGINE + 512 * S * H + 1024 * B * S * H + B * 256 * L + B * 256 * 16) + 15) & ~15


def _split(x, S: int, P: int):
    """[..., L] -> S + 2 segments [..., P]: index i + 1 holds x_i; x_{-1} and x_S are zero."""
    L = x.shape[-1]
    xp = F.pad(x, (P, (S + 1) * P - L))
    return [xp[..., i * P:(i + 1) * P] for i in range(S + 2)]


def _long_sums(g, k, dc, P: int):
    """c (without the skip term), dg (without it) and dk per read, by the formulas of csrc/hyena_longtrain.hip."""
    L = g.shape[-1]
    S, N = segments(L, P), 2 * P
    fft, ifft = (lambda t: torch.fft.fft(t, n=N)), (lambda t: torch.fft.ifft(t).real)
    gs, ks, ds = _split(g, S, P), _split(k, S, P), _split(dc, S, P)
    zero = torch.zeros_like(gs[0])
    K = [fft(ks[j + 1]) / N for j in range(S)]                                    # K_j = FFT([k_j ; 0]) / N
    X = [fft(torch.cat([gs[i], gs[i + 1]], -1)) for i in range(S)]                # X_i = FFT([g_{i-1} ; g_i])
    W = [fft(torch.cat([ds[m + 1], ds[m + 2]], -1)) for m in range(S)]            # W_m = FFT([dc_m ; dc_{m+1}])
    G = [fft(torch.cat([gs[m + 1], zero], -1)) for m in range(S)]                 # G_m = FFT([g_m ; 0])
    c, dg, dk = [], [], []
    for i in range(S):
        c.append(ifft(sum(X[i - j] * K[j] for j in range(i + 1)) * N)[..., P:])
        dg.append(ifft(sum(W[i + j] * K[j].conj() for j in range(S - i)) * N)[..., :P])
        dk.append(ifft(sum(W[m + i] * G[m].conj() for m in range(S - i)))[..., :P])
    cat = lambda parts: torch.cat(parts, -1)[..., :L]                            # noqa: E731
    return cat(c), cat(dg), cat(dk)


def segmented_core(zc, sw, sb, k, D, dy, P: int = P_ENGINE):
    """`hyena_train_reference.fft_core` with the three long sums through segments of P tokens; dk of the reads added in read order."""
    ch, L = zc.shape[1] // 3, zc.shape[-1]
    u, taps = R._short(zc, sw, sb)
    x0, x1, v = u.split(ch, dim=1)
    g = v * x1
    dc = dy * x0
    conv, corr, dkr = _long_sums(g, k, dc, P)
    c = conv + D[None, :, None] * g
    y = c * x0
    dx0 = dy * c
    dg = corr + D[None, :, None] * dc
    dk = torch.zeros_like(k)
    for b in range(zc.shape[0]):
        dk = dk + dkr[b]
    _, _, dk_abs = _long_sums(g.abs(), k.abs(), dc.abs(), P)
    dD, dD_abs = (dc * g).sum((0, 2)), (dc * g).abs().sum((0, 2))
    du = torch.cat([dx0, dg * v, dg * x1], dim=1)
    dup = F.pad(du, (0, 2))
    dzc = sum(sw[None, :, j, None] * dup[..., 2 - j:2 - j + L] for j in range(3))
    dsw, dsw_abs = (du[..., None] * taps).sum((0, 2)), (du[..., None] * taps).abs().sum((0, 2))
    dsb, dsb_abs = du.sum((0, 2)), du.abs().sum((0, 2))
    return {"c": c, "y": y, "dg": dg, "dzc": dzc, "dsw": dsw, "dsb": dsb, "dk": dk, "dD": dD,
            "den": {"dk": dk_abs.sum(0), "dD": dD_abs, "dsw": dsw_abs, "dsb": dsb_abs}}
