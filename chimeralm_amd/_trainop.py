"""What the training ops' Python wrappers share (cnntrain, mambatrain, tftrain, hyenatrain): the stream handed to a launch, inverted
dropout from a generator, the dtype / layout check in front of a launch and the text of an ABI return code."""
from __future__ import annotations

import ctypes as C

import torch

ABI_ERRORS = {-1: "CLM_E_INVALID: bad argument / shape", -2: "CLM_E_HIP: a HIP runtime call failed",
              -4: "CLM_E_UNSUPPORTED: shape or mode outside what the kernels cover"}


def abi_error(rc: int) -> str:
    """A negative return code of include/chimeralm_hip.h as its name and meaning."""
    return ABI_ERRORS.get(int(rc), f"error {rc}")


def stream_of(where) -> C.c_void_p:
    """torch's current stream on a device, or on a tensor's, as the ABI's `hipStream_t` argument."""
    device = where.device if isinstance(where, torch.Tensor) else where
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def inverted_dropout(t: torch.Tensor, p: float, generator: torch.Generator | None) -> torch.Tensor:
    """`t` with each element kept with probability 1 - p and scaled by 1 / (1 - p); the mask is drawn from `generator` (None:
    torch's default one).  At p <= 0 nothing is drawn and `t` itself comes back."""
    p = float(p)
    if p <= 0.0:
        return t
    keep = torch.rand(t.shape, device=t.device, generator=generator) >= p
    return t * (keep.to(t.dtype) * (1.0 / (1.0 - p)))


def is_plain_fp32(t: torch.Tensor, device: torch.device) -> bool:
    """What every training op takes: a contiguous fp32 tensor on `device`."""
    return t.dtype == torch.float32 and t.is_contiguous() and t.device == device
