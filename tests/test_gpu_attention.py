"""Self-attention kernel of the SequenceCNNTransformer encoder (csrc/attention.hip) against the oracle's attention
(oracle/transformer_oracle.py::attention, pinned to the reference module through the whole-model goldens)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import transformer_oracle as to

pytestmark = pytest.mark.gpu


def _run(qkv: torch.Tensor, prec: int) -> torch.Tensor:
    from chimeralm_amd import _native as N

    lib = N.load()
    B, L, _ = qkv.shape
    out = torch.empty((B, L, 256), dtype=qkv.dtype, device=qkv.device)
    rc = lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), B, L, prec,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _reference(qkv: torch.Tensor) -> torch.Tensor:
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, 8, 32).transpose(1, 2) for t in qkv.float().split(256, dim=-1))
    return to.attention(q, k, v).transpose(1, 2).reshape(B, L, 256)


@pytest.mark.parametrize("B,L", [(1, 1), (2, 31), (1, 64), (3, 65), (2, 128), (1, 129), (2, 1000), (1, 1024), (1, 4096)])
def test_attention_matches_oracle_fp16(built_lib, B, L):
    from chimeralm_amd import _native as N

    rng = np.random.default_rng(L * 7 + B)
    x = rng.standard_normal((B, L, 768)).astype(np.float32)
    x[..., :256] *= 1.5                                                       # sharper softmax than unit-variance scores
    x[0, L // 2, 256:512] *= 4.0                                              # one dominant key: exercises the running maximum
    qkv = torch.from_numpy(x).half()
    ref = _reference(qkv)
    got = _run(qkv.cuda(), N.PREC_F16).cpu().float()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err < 3e-3, f"max |attention - oracle| = {err:.2e}"
    again = _run(qkv.cuda(), N.PREC_F16).cpu().float()
    assert torch.equal(got, again)                                            # deterministic: fixed reduction order


def test_attention_bf16_and_arguments(built_lib):
    from chimeralm_amd import _native as N

    rng = np.random.default_rng(3)
    qkv = torch.from_numpy(rng.standard_normal((2, 300, 768)).astype(np.float32)).bfloat16()
    got = _run(qkv.cuda(), N.PREC_BF16).cpu().float()
    assert (got - _reference(qkv)).abs().max().item() < 2.5e-2
    lib = N.load()
    assert lib.clm_attention_fwd(None, None, 1, 1, N.PREC_F16, None) == N.E_INVALID
    assert lib.clm_attention_fwd(C.c_void_p(1), C.c_void_p(1), 1, 1, N.PREC_F32, None) == N.E_INVALID   # 16-bit only
    # ceil(L / 128) * 8 * B = 2^36 workgroups are more than a grid takes: refused by both entries before any launch (the pointers are
    # non-null and aligned, and never read)
    big = 1 << 20
    for prec in (N.PREC_F16, N.PREC_BF16, N.PREC_F16C):
        assert lib.clm_attention_fwd(C.c_void_p(16), C.c_void_p(16), big, big, prec, None) == N.E_INVALID
    for prec in (N.PREC_F32, N.PREC_F16X3):
        assert lib.clm_attention_exact_fwd(C.c_void_p(16), C.c_void_p(16), big, big, prec, None) == N.E_INVALID


# ---- the exact path's attention kernels (csrc/attention.hip attention32_kernel, attention_x3_kernel) through clm_attention_exact_fwd ---
# 128-query tiles, 64-key tiles: one key too many or too few at 4,096 positions moves an output by ~|v| / L = 2.4e-4, which the
# whole-model bounds (1e-4 on logits after 12 layers) cannot resolve -- here each kernel is held to an fp64 softmax(q k^T / sqrt(32)) v.
ATT32_TOL = {"fp32": 1e-5, "fp16x3": 2e-5}                  # absolute, unit-scale v: >= 10x below one miscounted key at 4,096
# ... or 1.5x what fp32 rounding of the scores alone costs, where that is more: scores of ~60 have an fp32 ulp of 3.8e-6, and torch's
# own fp32 attention is 1e-5 .. 3.2e-5 from fp64 on the "large" pattern (measured; the kernels: 1e-5 .. 2.9e-5).  Softmax rows that
# peaked put O(0.1) of their weight on single keys, so one miscounted key there moves an output far more than 2.4e-4.
ATT32_PATTERNS = ("normal", "ragged_max", "rising", "first_tile_max", "large")


def _qkv32(B: int, L: int, pattern: str) -> torch.Tensor:
    """fp32 [B, L, 768] whose scores s = q.k / sqrt(32) follow `pattern`; v unit-normal throughout."""
    rng = np.random.default_rng(1000 * L + 10 * B + ATT32_PATTERNS.index(pattern))
    x = rng.standard_normal((B, L, 768)).astype(np.float32)
    q, k = x[..., :256].reshape(B, L, 8, 32), x[..., 256:512].reshape(B, L, 8, 32)
    u = np.zeros(32, np.float32)
    u[0] = 1.0
    if pattern == "ragged_max":             # the last key (in the last key tile, ragged wherever L % 64 != 0) ~10 above all others
        d = rng.standard_normal((B, 1, 8, 32)).astype(np.float32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        q[:] = 0.3 * q + 2.0 * d
        k[:, L - 1] = 5.0 * np.sqrt(32.0) * d[:, 0]
    elif pattern == "rising":               # s = 0.01 * key index (+ noise): the running maximum moves on every key tile
        q[:] = 0.1 * q + u * np.sqrt(32.0)
        k[:] = 0.1 * k
        k[..., 0] = 0.01 * np.arange(L, dtype=np.float32)[None, :, None]
    elif pattern == "first_tile_max":       # the maximum among the first 64 keys, every later key at least 40 below it
        q[:] = 0.05 * q + u * np.sqrt(32.0)
        k[:] = 0.05 * k
        k[..., 0] = -45.0
        k[:, : min(L, 64), :, 0] = rng.uniform(-2.0, 2.0, (B, min(L, 64), 8))
    elif pattern == "large":                # |q| |k| / sqrt(32) = 100: the largest scores of a query at ~60
        q[:] = q / np.linalg.norm(q, axis=-1, keepdims=True) * np.sqrt(100.0 * np.sqrt(32.0))
        k[:] = k / np.linalg.norm(k, axis=-1, keepdims=True) * np.sqrt(100.0 * np.sqrt(32.0))
    return torch.from_numpy(x)


def _reference64(qkv: torch.Tensor) -> torch.Tensor:
    """`to.attention` in fp64, one (read, head) at a time (a 4,096-position score matrix is 134 MB in fp64)."""
    B, L, _ = qkv.shape
    x = qkv.double()
    out = torch.empty((B, L, 256), dtype=torch.float64)
    for b in range(B):
        for h in range(8):
            q, k, v = (x[b, :, o + 32 * h: o + 32 * h + 32][None, None] for o in (0, 256, 512))
            out[b, :, 32 * h: 32 * h + 32] = to.attention(q, k, v)[0, 0]
    return out


def _run32(qkv: torch.Tensor, prec: int) -> torch.Tensor:
    """clm_attention_exact_fwd into a buffer one read longer than [B, L, 256]; the NaN tail must come back untouched."""
    from chimeralm_amd import _native as N

    B, L, _ = qkv.shape
    buf = torch.full(((B + 1) * L * 256,), float("nan"), dtype=torch.float32, device="cuda")
    rc = N.load().clm_attention_exact_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(buf.data_ptr()), B, L, prec,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.isnan(out[B * L * 256:]).all(), "clm_attention_exact_fwd wrote past out[B * L * 256]"
    return out[: B * L * 256].reshape(B, L, 256)


@pytest.mark.parametrize("pattern", ATT32_PATTERNS)
@pytest.mark.parametrize("B,L", [(1, 1), (2, 63), (1, 64), (3, 65), (2, 127), (1, 128), (2, 129), (3, 513), (2, 1000), (1, 4095),
                                 (2, 4096), (1, 4097)])
def test_exact_attention_kernels_match_fp64(built_lib, B, L, pattern):
    from chimeralm_amd import _native as N

    qkv = _qkv32(B, L, pattern)
    ref = _reference64(qkv)
    floor = (_reference(qkv).double() - ref).abs().max().item()                  # the oracle's attention in fp32
    dev = qkv.cuda()
    msg = [f"fp32 oracle {floor:.2e}"]
    for name, prec in (("fp32", N.PREC_F32), ("fp16x3", N.PREC_F16X3)):
        got = _run32(dev, prec)
        assert torch.isfinite(got).all()
        err = (got.double() - ref).abs().max().item()
        msg.append(f"{name} {err:.2e}")
        tol = max(ATT32_TOL[name], 1.5 * floor)
        assert err <= tol, f"{name} {B} x {L} {pattern}: max |attention - fp64| = {err:.2e} > {tol:.2e} ({msg[0]})"
        assert torch.equal(got, _run32(dev, prec))                                # bitwise repeatable
    print(f"attention32 {B} x {L} {pattern}: " + ", ".join(msg))


def test_exact_attention_arguments(built_lib):
    from chimeralm_amd import _native as N

    lib = N.load()
    assert lib.clm_attention_exact_fwd(None, None, 1, 1, N.PREC_F32, None) == N.E_INVALID
    for prec in (N.PREC_F16, N.PREC_BF16, N.PREC_F16C):                         # fp32 operands: the exact path's two arithmetics only
        assert lib.clm_attention_exact_fwd(C.c_void_p(1), C.c_void_p(1), 1, 1, prec, None) == N.E_INVALID
    assert lib.clm_attention_exact_fwd(C.c_void_p(1), C.c_void_p(1), 0, 1, N.PREC_F32, None) == N.E_INVALID
    assert lib.clm_attention_exact_fwd(C.c_void_p(1), C.c_void_p(1), 1, 0, N.PREC_F16X3, None) == N.E_INVALID
    for prec in (N.PREC_F32, N.PREC_F16X3):                                     # the kernels read and write float4: 16-byte alignment
        assert lib.clm_attention_exact_fwd(C.c_void_p(8), C.c_void_p(16), 1, 1, prec, None) == N.E_INVALID
        assert lib.clm_attention_exact_fwd(C.c_void_p(16), C.c_void_p(8), 1, 1, prec, None) == N.E_INVALID
