"""fp64 reference, derived per-element error bound and a CPU emulation of the 16-bit self-attention kernel
(csrc/attention.hip attention_fwd_kernel<PREC, HILO>): modes "fp16", "bf16" and "hilo" (fp16 operands, the output as two fp16
planes hi = fp16(64 a), lo = fp16(64 a - hi), the transformer's fp16c mode).  CPU only; tests/test_attention16_host.py proves the
bound on the emulation, tests/test_gpu_attention16.py holds the kernel to it.

The bound.  Inputs are the 16-bit values themselves, so they carry no error.  For one read and head, query i, channel d, with w the
fp64 softmax weights, o = sum_j w_ij v_jd, A_id = sum_j w_ij |v_jd|, u the unit roundoff of the 16-bit type (2^-11 fp16, 2^-8 bf16):

    tol[i, d] = u A_id                    every p_ij is rounded to 16 bits (relative error <= u) before the second MFMA, while the
                                          denominator l sums the unrounded p: the weights of the numerator are each off by <= u
              + u_out |o_id|              the output's own rounding: u for the one-plane modes; hi + lo carries 11 + 11 bits, 2^-21
                                          of |o| (HILO is compared after (hi + lo) / 64 in fp64)
              + 2 eps_i A_id              a score is a 32-term fp32 dot product scaled by c = log2(e) / sqrt(32) in an FMA against
                                          the running maximum, then exp2: |d s_ij| <= 36 * 2^-24 * sum_d |q_id k_jd| / sqrt(32)
                                          (32 accumulations + FMA + the exponential's argument and result), eps_i its maximum over
                                          the keys; an error d s in the exponent moves p by a factor e^(d s), and it moves numerator
                                          and denominator in opposite directions at worst: 2 eps_i on the normalised weights
              + L 2^-24 A_id              fp32 accumulation of L products into o and of L terms into l, and one rescaling by alpha
                                          per 64-key tile of each: <= L roundings of 2^-24 between them, on weights summing to A_id
              + 2^-25 sum_j |v_jd|        fp16 only: p below 2^-14 is subnormal in fp16 and rounds ABSOLUTELY, by <= 2^-25; p is
                                          taken against a running maximum <= the final one, later factors alpha are <= 1 and the
                                          final l is >= 1 (the maximal key has p = 1), so each key's normalised weight is off by
                                          <= 2^-25 whatever its size.  bf16 has fp32's exponent range: no such term.

Derived, not fitted; no safety factor.  A test asserts max(err / tol) <= 1."""
from __future__ import annotations

import math

import torch

HD, NH, D = 32, 8, 256
KT = 64                                     # keys per tile of the kernel's online softmax
HILO_SCALE = 64.0                           # ATT_HILO_SCALE
MODES = ("fp16", "bf16", "hilo")
DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "hilo": torch.float16}
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "hilo": 2.0 ** -11}
U_OUT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "hilo": 2.0 ** -21}


def round_inputs(qkv32: torch.Tensor, mode: str) -> torch.Tensor:
    """The fp32 pattern rounded to the mode's 16-bit operand type: what the kernel is given and what the reference starts from."""
    return qkv32.to(DTYPE[mode])


def reference_and_bound(qkv16: torch.Tensor, mode: str, with_dropped: bool = False):
    """(ref, tol): the fp64 softmax(q k^T / sqrt(32)) v of the 16-bit inputs and the bound of the module docstring, both [B, L, 256]
    fp64, one (read, head) at a time (a 4,096-position score matrix is 134 MB in fp64).  `with_dropped` adds a third tensor: the
    same attention with key L - 1 left out (L >= 2), what a kernel that miscounts the ragged tile would compute."""
    assert qkv16.dtype == DTYPE[mode]
    B, L, _ = qkv16.shape
    x = qkv16.double()
    out = torch.empty((B, L, D), dtype=torch.float64)
    tol = torch.empty((B, L, D), dtype=torch.float64)
    dropped = torch.empty((B, L, D), dtype=torch.float64) if with_dropped else None
    u, u_out = U[mode], U_OUT[mode]
    for b in range(B):
        for h in range(NH):
            q, k, v = (x[b, :, o + HD * h: o + HD * h + HD] for o in (0, D, 2 * D))
            s = (q @ k.T) / math.sqrt(HD)
            w = torch.softmax(s, dim=-1)
            o = w @ v
            a = w @ v.abs()
            eps = 36.0 * 2.0 ** -24 * (q.abs() @ k.abs().T).amax(dim=1, keepdim=True) / math.sqrt(HD)
            t = (u + 2.0 * eps + L * 2.0 ** -24) * a + u_out * o.abs()
            if u == 2.0 ** -11:
                t = t + 2.0 ** -25 * v.abs().sum(dim=0, keepdim=True)
            out[b, :, HD * h: HD * h + HD] = o
            tol[b, :, HD * h: HD * h + HD] = t
            if with_dropped:
                dropped[b, :, HD * h: HD * h + HD] = torch.softmax(s[:, : L - 1], dim=-1) @ v[: L - 1]
    return (out, tol, dropped) if with_dropped else (out, tol)


def hilo_bound(ref: torch.Tensor, tol_fp16: torch.Tensor) -> torch.Tensor:
    """The "hilo" bound from the "fp16" one of the same operands: only the output-rounding term differs (2^-21 for 2^-11)."""
    return tol_fp16 - (U_OUT["fp16"] - U_OUT["hilo"]) * ref.abs()


def emulate(qkv16: torch.Tensor, mode: str) -> torch.Tensor:
    """The kernel's arithmetic on the CPU: fp32 scores, online softmax over 64-key tiles with p = exp2(s c - m c), p rounded to the
    16-bit type before p @ v, fp32 accumulation rescaled by alpha, l from the unrounded p, one final division, output rounding.
    Returns [B, L, 256] in the 16-bit type, or for "hilo" [2, B, L, 256] fp16: the hi plane, then the lo plane."""
    dt = DTYPE[mode]
    assert qkv16.dtype == dt
    B, L, _ = qkv16.shape
    c = torch.tensor(1.4426950408889634 * 0.17677669529663687, dtype=torch.float32)
    x = qkv16.float().reshape(B, L, 3, NH, HD).permute(2, 0, 3, 1, 4)              # [3, B, 8, L, 32]
    q, k, v = x[0], x[1], x[2]
    m = torch.full((B, NH, L, 1), -math.inf, dtype=torch.float32)
    l = torch.zeros((B, NH, L, 1), dtype=torch.float32)
    o = torch.zeros((B, NH, L, HD), dtype=torch.float32)
    for k0 in range(0, L, KT):
        s = q @ k[:, :, k0: k0 + KT].transpose(-1, -2)                            # fp32 products of 16-bit values, fp32 sums
        m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * c)
        p = torch.exp2(s * c - m_new * c)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        o = o * alpha + p.to(dt).float() @ v[:, :, k0: k0 + KT]
        m = m_new
    inv = 1.0 / l
    if mode == "hilo":
        y = (o * (inv * HILO_SCALE)).transpose(1, 2).reshape(B, L, D)
        hi = y.half()
        return torch.stack((hi, (y - hi.float()).half()))
    return (o * inv).transpose(1, 2).reshape(B, L, D).to(dt)


def to_float64(got: torch.Tensor, mode: str) -> torch.Tensor:
    """The kernel's (or the emulation's) output as fp64 [B, L, 256]; HILO is reconstructed as (hi + lo) / 64."""
    if mode == "hilo":
        return (got[0].double() + got[1].double()) / HILO_SCALE
    return got.double()


def worst_ratio(got64: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """max over elements of |got - ref| / tol; inf where got is not finite."""
    if not torch.isfinite(got64).all():
        return math.inf
    err = (got64 - ref).abs()
    return torch.where(err == 0, err, err / tol).max().item()                     # an exact element passes a zero bound


def ulp16(x: torch.Tensor, mode: str) -> torch.Tensor:
    """The spacing of the mode's 16-bit type at each value of x (the type's own, or fp64 holding such values), as fp64."""
    e = torch.frexp(x.double())[1].double()                                       # x = m 2^e with 0.5 <= |m| < 1
    if DTYPE[mode] == torch.bfloat16:
        return torch.exp2(e - 8.0)
    return torch.where(x == 0, torch.full_like(e, 2.0 ** -24), torch.exp2((e - 11.0).clamp(min=-24.0)))


def check_hilo_planes(hi: torch.Tensor, lo: torch.Tensor, plain: torch.Tensor | None = None) -> None:
    """What the two fp16 planes of one HILO output promise: lo is the rounded remainder of hi, so |lo| <= ulp(hi) / 2 and
    fp16(float(hi) + float(lo)) gives hi back bit for bit -- except on the one tie that is correct behaviour: a remainder just below
    half an ulp rounds, as an fp16 value of its own, UP to exactly ulp(hi) / 2; hi + lo then lies midway between hi and its neighbour
    and round-to-nearest-EVEN leaves an odd hi (5 of 66,048 elements of the emulation at 2 x 129).  Those elements must be exactly
    that: |lo| == ulp(hi) / 2 and hi's last mantissa bit set.  `plain`, the one-plane fp16 output on the same input: hi is within
    one fp16 ulp of 64 * plain (the same fp32 value scaled by a power of two, rounded once) -- where plain is subnormal in fp16
    (|a| < 2^-14) it was rounded on a grid 64 times coarser than hi's, and its own half spacing, 64 * 2^-25, is allowed on top."""
    assert hi.dtype == lo.dtype == torch.float16
    ulp = ulp16(hi, "hilo")
    assert (lo.double().abs() <= ulp / 2).all(), "HILO: |lo| > ulp(hi) / 2"
    back = (hi.float() + lo.float()).half()
    same = back.view(torch.int16) == hi.view(torch.int16)
    tie = (lo.double().abs() == ulp / 2) & ((hi.view(torch.int16) & 1) == 1)
    assert (same | tie).all(), f"HILO: fp16(hi + lo) != hi on {(~(same | tie)).sum().item()} elements that are no rounding tie"
    if plain is not None:
        slack = torch.where(plain.double().abs() < 2.0 ** -14, HILO_SCALE * 2.0 ** -25, 0.0)
        assert ((hi.double() - HILO_SCALE * plain.double()).abs() <= ulp + slack).all(), "HILO: hi is not the fp16 output x 64"


def counting_case(B: int, L: int, mode: str):
    """q = k = 0 (every p exactly 1, l exactly L) and read b marking key j = 256 b + ch with v[b, j, ch] = 1, all other v 0: channel
    ch of EVERY query row of read b is then 1 / L if key j exists (j < L) and 0 if not.  A dropped key gives 0 for 1 / L, a clone of
    key L - 1 counted in the ragged tile 2 / L or more.  Returns (qkv [B, L, 768] 16-bit, marked [B, 256] bool)."""
    qkv = torch.zeros((B, L, 3 * D), dtype=DTYPE[mode])
    j = 256 * torch.arange(B)[:, None] + torch.arange(D)[None, :]                 # [B, 256]: the key that (read, channel) marks
    marked = j < L
    bb, cc = marked.nonzero(as_tuple=True)
    qkv[bb, j[bb, cc], 2 * D + cc] = 1.0
    return qkv, marked


def check_counting(got: torch.Tensor, marked: torch.Tensor, L: int, mode: str) -> float:
    """`got` ([B, L, 256], or the two planes for "hilo", on any device) against `counting_case`: exactly 0 where the marked key does
    not exist; where it does, within one 16-bit ulp of the 16-bit rounding of 1 / L, or for "hilo" (hi + lo) / 64 within 2^-20 of
    1 / L relatively.  Returns the worst deviation from 1 / L in units of what is allowed."""
    x = to_float64(got, mode)
    mk = marked.to(x.device)[:, None, :].expand_as(x)
    assert (x[~mk] == 0).all(), f"{mode} L={L}: a channel whose marked key is past the read is not exactly 0"
    if mode == "hilo":
        want, allowed = torch.tensor(1.0 / L, dtype=torch.float64), 2.0 ** -20 / L
    else:
        want = torch.tensor(1.0 / L, dtype=torch.float64).to(DTYPE[mode]).double()
        allowed = ulp16(want, mode).item()
    dev = ((x[mk] - want.to(x.device)).abs() / allowed).max().item() if mk.any() else 0.0
    assert dev <= 1.0, f"{mode} L={L}: a marked key's channel is {dev:.3g} x the allowed distance from 1 / L: miscounted keys"
    return dev
