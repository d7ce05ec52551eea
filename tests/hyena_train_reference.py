"""Reference arithmetic for the Hyena training core (csrc/hyena_train.hip, chimeralm_amd/hyenatrain.py).  TEST INFRASTRUCTURE.

* `autograd_core`: the operator through `hyena_oracle.short_filter`'s conv1d and `hyena_oracle.fftconv`, differentiated by torch.
* `hand_core`: the formulas of DESIGN.md 5.15 written out, dtype-generic (float64: the truth; float32 on the CPU: the yardstick of the
  project's bound), with the denominators of the batch-reduced gradients (the sums of the absolute terms).
* `circular_pairs`: the circular form at N >= 2 L - 2 with two READS packed as real / imaginary part, its three alias corrections and
  the `Re IFFT(X conj Y)` identity for dk.
* `circular_mirror`: the form the kernels run -- two real sequences of ONE read packed, separated through the mirrored bin -- with
  the kernels' balancing of the two packed sequences, every output of the op, and `DEFECTS`: wrong variants planted by
  tests/test_grad_rows_host.py into the float32 evaluation only.
* `net_step`: one training step of the whole net in torch autograd over `hyena_oracle.backbone_forward` + `head_forward`.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import hyena_oracle as ho

C = ho.D_MODEL
CORE_GRADS = ("dzc", "dsw", "dsb", "dk", "dD")
# no_alias: the three corrections at N == 2 L - 2 left out | unbalanced: the two sequences of a transform packed as they come |
# short_tail: the transposed 3-tap filter reads du[L - 2] and du[L - 1] as 0
DEFECTS = ("no_alias", "unbalanced", "short_tail")


def logn_for(L: int) -> int:
    """csrc/hyena_conv.hip conv_logn_for."""
    for logn in range(8, 15):
        if 2 * L - 2 <= (1 << logn):
            return logn
    return -1


def workspace_bytes(B: int, L: int) -> int:
    """The formula of include/chimeralm_hip.h."""
    n = 1 << logn_for(L)
    return (4 * (n + 512 * (n // 2 + 1) + B * 256 * L + B * 256 * 16) + 15) & ~15


def random_core(seed: int, B: int, L: int, dtype=torch.float32, channels: int = C, decaying_filter: bool = False):
    """zc, sw, sb, k, D, dy of one call (fp32 values, cast to `dtype`)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    zc, sw, sb = r(B, 3 * channels, L), r(3 * channels, 3) * 0.5, r(3 * channels) * 0.5
    if decaying_filter:
        k = ho.hyena_filter(ho.make_state_dict(seed), 0, L).t().contiguous()[:channels]
    else:
        k = r(channels, L)
    D, dy = r(channels), r(B, channels, L)
    return tuple(t.to(dtype) for t in (zc, sw, sb, k, D, dy))


def autograd_core(zc, sw, sb, k, D, dy):
    """c-less truth: y and the five gradients through conv1d and `fftconv`."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (zc, sw, sb, k, D)]
    z, w, b, kk, dd = leaves
    L = z.shape[-1]
    uc = F.conv1d(z, w.unsqueeze(1), b, padding=2, groups=z.shape[1])[..., :L]
    x0, x1, v = uc.split(z.shape[1] // 3, dim=1)
    y = ho.fftconv(v * x1, kk, dd) * x0
    y.backward(dy)
    out = {"y": y.detach()}
    out.update({n: t.grad for n, t in zip(CORE_GRADS, leaves)})
    return out


def _short(zc, sw, sb):
    L = zc.shape[-1]
    zp = F.pad(zc, (2, 0))
    taps = torch.stack([zp[..., j:j + L] for j in range(3)], dim=-1)              # zc[r, t - 2 + j]
    return (taps * sw[None, :, None, :]).sum(-1) + sb[None, :, None], taps


def _toeplitz(k):
    """T[ch, t, s] = k[ch, t - s] for t >= s, else 0."""
    L = k.shape[-1]
    idx = torch.arange(L)[:, None] - torch.arange(L)[None, :]
    return torch.where(idx >= 0, k[:, idx.clamp_min(0)], torch.zeros((), dtype=k.dtype))


def hand_core(zc, sw, sb, k, D, dy):
    """The written formulas as dense sums in the tensors' own dtype -> c, y, the five gradients and `den`: for dk, dD, dsw, dsb the
    sums of the absolute terms."""
    ch = zc.shape[1] // 3
    u, taps = _short(zc, sw, sb)
    x0, x1, v = u.split(ch, dim=1)
    g = v * x1
    T = _toeplitz(k)                                                               # [ch, t, s]
    c = torch.einsum("cts,bcs->bct", T, g) + D[None, :, None] * g
    y = c * x0
    dc, dx0 = dy * x0, dy * c
    dg = torch.einsum("cts,bct->bcs", T, dc) + D[None, :, None] * dc
    L = zc.shape[-1]
    idx = torch.arange(L)[:, None] - torch.arange(L)[None, :]                      # t - tau
    gs = torch.where(idx >= 0, g[..., idx.clamp_min(0)], torch.zeros((), dtype=g.dtype))     # g[b, c, t - tau]
    dk = torch.einsum("bct,bctu->cu", dc, gs)
    dk_abs = torch.einsum("bct,bctu->cu", dc.abs(), gs.abs())
    dD, dD_abs = (dc * g).sum((0, 2)), (dc * g).abs().sum((0, 2))
    du = torch.cat([dx0, dg * v, dg * x1], dim=1)
    dup = F.pad(du, (0, 2))
    dzc = sum(sw[None, :, j, None] * dup[..., 2 - j:2 - j + L] for j in range(3))
    dsw, dsw_abs = (du[..., None] * taps).sum((0, 2)), (du[..., None] * taps).abs().sum((0, 2))
    dsb, dsb_abs = du.sum((0, 2)), du.abs().sum((0, 2))
    return {"c": c, "y": y, "dg": dg, "dzc": dzc, "dsw": dsw, "dsb": dsb, "dk": dk, "dD": dD,
            "den": {"dk": dk_abs, "dD": dD_abs, "dsw": dsw_abs, "dsb": dsb_abs}}


def fft_core(zc, sw, sb, k, D, dy):
    """`hand_core`'s formulas with every long sum through `rfft` / `irfft` at n = 2 L (as `fftconv`), in the tensors' own dtype: the
    reference of the full-width GPU cases (float64) and their float32-on-the-CPU yardstick.  Same keys as `hand_core`."""
    ch, L = zc.shape[1] // 3, zc.shape[-1]
    n = 2 * L
    rf = lambda t: torch.fft.rfft(t, n=n)                                         # noqa: E731
    conv = lambda a, b_: torch.fft.irfft(rf(a) * rf(b_), n=n)[..., :L]            # noqa: E731  sum_s a[s] b[t - s]
    corr = lambda a, b_: torch.fft.irfft(rf(a) * rf(b_).conj(), n=n)[..., :L]     # noqa: E731  sum_t a[t] b[t - s]
    u, taps = _short(zc, sw, sb)
    x0, x1, v = u.split(ch, dim=1)
    g = v * x1
    c = conv(g, k) + D[None, :, None] * g
    y = c * x0
    dc, dx0 = dy * x0, dy * c
    dg = corr(dc, k) + D[None, :, None] * dc
    dk, dk_abs = corr(dc, g).sum(0), corr(dc.abs(), g.abs()).sum(0)
    dD, dD_abs = (dc * g).sum((0, 2)), (dc * g).abs().sum((0, 2))
    du = torch.cat([dx0, dg * v, dg * x1], dim=1)
    dup = F.pad(du, (0, 2))
    dzc = sum(sw[None, :, j, None] * dup[..., 2 - j:2 - j + L] for j in range(3))
    dsw, dsw_abs = (du[..., None] * taps).sum((0, 2)), (du[..., None] * taps).abs().sum((0, 2))
    dsb, dsb_abs = du.sum((0, 2)), du.abs().sum((0, 2))
    return {"c": c, "y": y, "dg": dg, "dzc": dzc, "dsw": dsw, "dsb": dsb, "dk": dk, "dD": dD,
            "den": {"dk": dk_abs, "dD": dD_abs, "dsw": dsw_abs, "dsb": dsb_abs}}


def _fftn(t, n):
    return torch.fft.fft(t, n=n)


def circular_pairs(zc, sw, sb, k, D, dy, n: int | None = None):
    """c, dg and dk through circular transforms of n >= 2 L - 2 points (default: exactly 2 L - 2, the alias case) with two reads
    packed as real / imaginary part (an odd B leaves the last imaginary part zero) and the three alias corrections."""
    B, L, ch = zc.shape[0], zc.shape[-1], zc.shape[1] // 3
    n = max(2 * L - 2, L) if n is None else n
    alias = n == 2 * L - 2 and L > 1
    u, _ = _short(zc, sw, sb)
    x0, x1, v = u.split(ch, dim=1)
    g = v * x1
    K = _fftn(k, n)
    zero = torch.zeros_like(g[0])
    c, dk = torch.zeros_like(g), torch.zeros_like(k)
    for p in range(0, B, 2):
        gb = g[p + 1] if p + 1 < B else zero
        r = torch.fft.ifft(_fftn(torch.complex(g[p], gb), n) * K)[..., :L]
        c[p] = r.real
        if p + 1 < B:
            c[p + 1] = r.imag
    if alias:
        c[..., 0] -= g[..., L - 1] * k[..., L - 1]
    c = c + D[None, :, None] * g
    dc = dy * x0
    dg = torch.zeros_like(g)
    for p in range(0, B, 2):
        db, gb = (dc[p + 1], g[p + 1]) if p + 1 < B else (zero, zero)
        X, Y = _fftn(torch.complex(dc[p], db), n), _fftn(torch.complex(g[p], gb), n)
        r = torch.fft.ifft(X * K.conj())[..., :L]
        dg[p] = r.real
        if p + 1 < B:
            dg[p + 1] = r.imag
        dk += torch.fft.ifft(X * Y.conj()).real[..., :L]                           # the cross terms land in the imaginary part
    if alias:
        dg[..., L - 1] -= dc[..., 0] * k[..., L - 1]
        dk[..., L - 1] -= (dc[..., 0] * g[..., L - 1]).sum(0)
    return {"c": c, "dg": dg + D[None, :, None] * dc, "dk": dk}


def _balance(a, b):
    """csrc/hyena_train.hip hyena_train_balance per sequence pair: the power of two that brings b's sum of squares to a's."""
    n1, n2 = a.pow(2).sum(-1, keepdim=True), b.pow(2).sum(-1, keepdim=True)
    ok = (n1 > 0) & (n2 > 0) & torch.isfinite(n1) & torch.isfinite(n2)
    one = torch.ones_like(n1)
    sh = torch.div(torch.frexp(torch.where(ok, n1, one))[1] - torch.frexp(torch.where(ok, n2, one))[1], 2, rounding_mode="trunc")
    return torch.ldexp(one, sh.clamp(-40, 40))


def _split_spectra(Z):
    """A, B of Z = FFT(a + i b), a and b real: A[m] = (Z[m] + conj Z[n - m]) / 2, B[m] = (Z[m] - conj Z[n - m]) / 2i."""
    Zr = torch.roll(Z.flip(-1), 1, -1).conj()
    return (Z + Zr) / 2, (Z - Zr) / 2j


def circular_mirror(zc, sw, sb, k, D, dy, n: int | None = None, defect: str | None = None):
    """The kernels' form: per read, c of two channels from one transform and (dg, dk of the read) from one transform of dc + i g,
    the imaginary sequence of each packing scaled by `_balance` (inputs in the time domain, product spectra by Parseval) and the dk
    rows of the reads summed in read order.  Same keys as `hand_core`, without `den`.  `defect`: one of DEFECTS, planted."""
    L, ch = zc.shape[-1], zc.shape[1] // 3
    n = max(2 * L - 2, L) if n is None else n
    alias = n == 2 * L - 2 and L > 1 and defect != "no_alias"
    bal = (lambda a, b_: torch.ones_like(a[..., :1])) if defect == "unbalanced" else _balance
    spec_norm = lambda S: (S.real ** 2 + S.imag ** 2)                              # noqa: E731
    u, taps = _short(zc, sw, sb)
    x0, x1, v = u.split(ch, dim=1)
    g = v * x1
    K = _fftn(k, n)
    rin = bal(g[:, 0::2], g[:, 1::2])
    A, Bs = _split_spectra(_fftn(torch.complex(g[:, 0::2], g[:, 1::2] * rin), n))
    S1, S2 = A * K[0::2], Bs * K[1::2]
    rout = bal(spec_norm(S1).sqrt(), spec_norm(S2).sqrt())
    r = torch.fft.ifft(S1 + 1j * S2 * rout)[..., :L]
    c = torch.zeros_like(g)
    c[:, 0::2], c[:, 1::2] = r.real, r.imag / (rin * rout)
    dc = dy * x0
    rin = bal(dc, g)
    X, Y = _split_spectra(_fftn(torch.complex(dc, g * rin), n))
    S1, S2 = X * K.conj(), X * Y.conj()
    rout = bal(spec_norm(S1).sqrt(), spec_norm(S2).sqrt())
    r = torch.fft.ifft(S1 + 1j * S2 * rout)[..., :L]
    dg, dkr = r.real.clone(), r.imag / (rin * rout)
    if alias:
        c[..., 0] -= g[..., L - 1] * k[..., L - 1]
        dg[..., L - 1] -= dc[..., 0] * k[..., L - 1]
        dkr[..., L - 1] -= dc[..., 0] * g[..., L - 1]
    dk = torch.zeros_like(k)
    for b in range(zc.shape[0]):                                                   # read order
        dk = dk + dkr[b]
    c, dg = c + D[None, :, None] * g, dg + D[None, :, None] * dc
    du = torch.cat([dy * c, dg * v, dg * x1], dim=1)
    dup = F.pad(du, (0, 2))
    if defect == "short_tail":
        dup[..., L - 2:L] = 0
    dzc = sum(sw[None, :, j, None] * dup[..., 2 - j:2 - j + L] for j in range(3))
    return {"c": c, "y": c * x0, "dg": dg, "dzc": dzc, "dsw": (du[..., None] * taps).sum((0, 2)), "dsb": du.sum((0, 2)), "dk": dk,
            "dD": (dc * g).sum((0, 2))}


# ------------------------------------------------------------------------------------------------------------- the net
def step_batch(seed: int = 5, B: int = 3, L: int = 203, pads: int = 17):
    """ids [B, L] (A/C/G/T, [SEP] last, `pads` left pads = 4 on read 0) and labels."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(7, 11, (B, L), generator=g)
    ids[:, -1] = 1
    ids[0, :pads] = 4
    return ids, torch.arange(B) % 2


def net_step(sd, ids, labels, dtype=torch.float64):
    """Loss, logits and every gradient (keyed as the module's `named_parameters`, without `net.`) of one step by torch autograd over
    the oracle's forward.  The three `freq` aliases are one leaf; its gradient is reported under `.1.freq`."""
    leaves = {}
    for k_, v_ in sd.items():
        t = v_.to(dtype)
        if k_.endswith((".implicit_filter.3.freq", ".implicit_filter.5.freq")):
            continue
        if k_.endswith((".pos_emb.t", ".modulation.deltas")):
            leaves[k_] = t
        else:
            leaves[k_] = t.clone().requires_grad_(True)
    full = dict(leaves)
    for k_ in sd:
        if k_.endswith((".implicit_filter.3.freq", ".implicit_filter.5.freq")):
            full[k_] = leaves[k_.replace(".3.freq", ".1.freq").replace(".5.freq", ".1.freq")]
    trace = {}
    logits = ho.head_forward(ho.backbone_forward(ids.long(), full, dtype), full, dtype, trace)
    trace["attn_weights"].retain_grad()
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    a, da = trace["attn_weights"].detach(), trace["attn_weights"].grad
    dscores = a * (da - (a * da).sum(dim=1, keepdim=True))                         # the softmax's backward
    grads = {k_[len("net."):]: (t.grad if t.grad is not None else torch.zeros_like(t)) for k_, t in leaves.items() if t.requires_grad}
    # the score bias shifts every score of a read alike and the softmax does not see it: its gradient, the sum of the score
    # gradients, is 0 up to rounding.  Its denominator is the sum of their absolute values, as for every cancelling sum here.
    den = {"head.attention.2.bias": dscores.abs().sum().reshape(1)}
    return {"loss": loss.detach(), "logits": logits.detach(), "grads": grads, "den": den}
