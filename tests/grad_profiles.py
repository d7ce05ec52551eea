"""Profiles of the gradient that reaches a training core, for tests/test_grad_rows_host.py and tests/test_gpu_grad_rows.py.

The existing training tests feed the backward a `dout` / `dy` that is unit-normal everywhere, so every row of every gradient has the
same size.  A real step's gradient comes through attention pooling, a max-pool route or a quality mask and spans many decades along a
read, between channels and between reads.  `factors(name, B, L, C)` is the fp32 factor that shapes a unit-normal gradient that way,
as a tensor broadcastable to [B, L, C].  Every factor is an exact power of two (or 0), so the scaling itself rounds nothing:

    uniform      1: the input of the existing tests
    ramp_down    2^-(t // 8), the exponent capped at RAMP_CAP;  ramp_up: its mirror in t
    rows3        1 at t = 0, L // 2 and L - 1, 0 elsewhere
    last_chunk   1 inside the last (ragged) chunk of Q tokens, 0 elsewhere;  first_chunk: 1 inside the first      (Mamba)
    channels     2^-(c mod 13): different scales on the two partners of every packed transform                      (Hyena)
    reads        2^-(10 b), the power of two next to 10^-(3 b): the batch-reduced sums, the independence of the reads

RAMP_CAP = 64: a unit-normal sample times 2^-64 and two further factors of a backward product (a probability, a key) stay inside
fp32's normal range; a deeper ramp (2^-128 at t = 1031) would make the scaled input itself subnormal, the scaling would round, and
the comparison would measure who flushes subnormals, not the kernel.
"""
from __future__ import annotations

import torch

RAMP_CAP = 64
TIME_PROFILES = ("uniform", "ramp_down", "ramp_up", "rows3", "last_chunk", "first_chunk")
PROFILES = TIME_PROFILES + ("channels", "reads")


def factors(name: str, B: int, L: int, C: int, Q: int = 64) -> torch.Tensor:
    """fp32, broadcastable to [B, L, C]."""
    t = torch.arange(L)
    if name == "uniform":
        return torch.ones(1, 1, 1)
    if name in ("ramp_down", "ramp_up"):
        e = torch.clamp(t // 8, max=RAMP_CAP)
        f = torch.ldexp(torch.ones(L), -e)
        return (f if name == "ramp_down" else f.flip(0)).reshape(1, L, 1)
    if name == "rows3":
        f = torch.zeros(L)
        f[[0, L // 2, L - 1]] = 1.0
        return f.reshape(1, L, 1)
    if name in ("last_chunk", "first_chunk"):
        c0 = (L - 1) // Q * Q if name == "last_chunk" else 0
        return ((t >= c0) & (t < c0 + Q)).float().reshape(1, L, 1)
    if name == "channels":
        return torch.ldexp(torch.ones(C), -(torch.arange(C) % 13)).reshape(1, 1, C)
    if name == "reads":
        return torch.ldexp(torch.ones(B), -10 * torch.arange(B)).reshape(B, 1, 1)
    raise ValueError(name)


def support(name: str, L: int, Q: int = 64) -> torch.Tensor:
    """bool [L]: the positions where the profile is non-zero."""
    return factors(name, 1, L, 1, Q).reshape(-1).expand(L) != 0
