"""The training attention op on the MI355X (csrc/attention_train.hip, `clm_attn_train_*`): the forward against the inference kernel
bit for bit, the keep mask against its numpy restatement, forward and backward against the fp64 formulas, counting probes,
independence of the reads, determinism, the extents written and the refusals.

Bound of every comparison (the project's, tests/test_gpu_mamba_train.py): max|engine - fp64| / max|fp64| <= max(8 x the same error of
the same formulas evaluated in float32 on the CPU, 32 x 2^-24).  CLM_ATTN_TRAIN_PARITY=<file> appends the measured ratios to that
file (profiles/attn_train_parity.txt is one such run).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import attention_train_reference as R

pytestmark = pytest.mark.gpu
FLOOR = 32 * 2.0 ** -24
LN2 = math.log(2.0)
# (B, L) at the smallest sizes where a tile edge exists: one position | inside one 32-row block | its edges | the 64-row streamed
# tile's edges | the 128-row owned tile's edges | several reads over ragged tiles | many tiles, more than one workgroup per (read, head)
SHAPES = [(1, 1), (2, 2), (2, 31), (2, 32), (2, 33), (2, 63), (2, 64), (2, 65), (1, 127), (2, 128), (1, 129), (3, 200), (2, 1031)]
TAIL = 16                                   # floats (64 bytes) of sentinel behind every output
SEED = 0x1234567887654321


def _lib():
    from chimeralm_amd import _native as N

    return N.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buf(n: int) -> torch.Tensor:
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")


def _take(buf: torch.Tensor, shape, what: str) -> torch.Tensor:
    n = int(np.prod(shape))
    assert torch.isnan(buf[n:]).all(), f"{what}: bytes past its end were written"
    return buf[:n].reshape(shape)


def _forward(qkv: torch.Tensor, p: float, seed: int = SEED):
    """clm_attn_train_forward on GPU qkv -> out [B, L, 256], lse [B, 8, L] (log2 units); the 64 bytes behind each stay untouched."""
    B, L, _ = qkv.shape
    out, lse = _buf(B * L * 256), _buf(B * 8 * L)
    rc = _lib().clm_attn_train_forward(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, p, seed, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _take(out, (B, L, 256), "out"), _take(lse, (B, 8, L), "lse")


def _backward(qkv, out, lse, dout, p: float, seed: int = SEED) -> torch.Tensor:
    B, L, _ = qkv.shape
    n = int(_lib().clm_attn_train_workspace_bytes(B, L))
    assert n == (4 * B * 8 * L + 15) // 16 * 16
    ws = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    dqkv = _buf(B * L * 768)
    rc = _lib().clm_attn_train_backward(qkv.data_ptr(), out.contiguous().data_ptr(), lse.contiguous().data_ptr(), dout.data_ptr(),
                                        dqkv.data_ptr(), ws.data_ptr(), B, L, p, seed, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((ws[n:] == 0x5A).all()), "workspace: bytes past its end were written"
    return _take(dqkv, (B, L, 768), "dqkv")


def _run(qkv_cpu, dout_cpu, p, seed=SEED):
    qkv, dout = qkv_cpu.cuda(), dout_cpu.cuda()
    out, lse = _forward(qkv, p, seed)
    d = _backward(qkv, out, lse, dout, p, seed)
    return {"out": out, "lse": lse, "dq": d[..., :256], "dk": d[..., 256:512], "dv": d[..., 512:], "dqkv": d}


def _exact(qkv: torch.Tensor) -> torch.Tensor:
    from chimeralm_amd import _native as N

    B, L, _ = qkv.shape
    out = torch.empty((B, L, 256), dtype=torch.float32, device="cuda")
    assert _lib().clm_attention_exact_fwd(qkv.data_ptr(), out.data_ptr(), B, L, N.PREC_F32, _stream()) == 0
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------------------- forward, bit for bit
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_without_dropout_is_the_inference_kernel(built_lib, B, L):
    for pattern in R.PATTERNS:
        qkv = R.make_qkv(B, L, pattern).cuda()
        out, lse = _forward(qkv, 0.0)
        assert torch.equal(out, _exact(qkv)), pattern
        assert bool(torch.isfinite(lse).all()), pattern


# ------------------------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("B,L", [(3, 200), (2, 65)])
def test_mask_is_the_numpy_mask(built_lib, B, L):
    from chimeralm_amd import tftrain

    for p in (0.1, 0.5):
        for seed in (SEED, 7):
            got = tftrain.attention_mask(B, L, p, seed, "cuda")
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().astype(bool), R.keep_mask(seed, B, L, p)), (p, seed)
    assert bool(tftrain.attention_mask(B, L, 0.0, SEED, "cuda").all())


# ------------------------------------------------------------------------------------------------------------- parity
def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def _check(tag, items):
    """items: (name, engine, fp64, fp32-on-CPU).  Prints every figure, then asserts them all."""
    rows, bad = [], []
    for name, got, r64, r32 in items:
        d = float(r64.abs().max().clamp_min(1e-300))
        err = float((got.double().cpu() - r64).abs().max()) / d
        err32 = float((r32.double() - r64).abs().max()) / d
        rows.append(f"{tag:34s} {name:4s} engine {err:.3e}  cpu-fp32 {err32:.3e}  bound {_bound(err32):.3e}  ratio {err / _bound(err32):.3f}")
        if not (np.isfinite(err) and err <= _bound(err32)):
            bad.append(rows[-1])
    print("\n".join(rows))
    if os.environ.get("CLM_ATTN_TRAIN_PARITY"):
        with open(os.environ["CLM_ATTN_TRAIN_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")
    return bad


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_parity_with_fp64(built_lib, B, L, pattern):
    qkv, dout = R.make_qkv(B, L, pattern), R.make_dout(B, L)
    bad = []
    for p in (0.0, 0.1, 0.5):
        keep = None if p == 0.0 else torch.from_numpy(R.keep_mask(SEED, B, L, p))
        r64, r32 = R.backward(qkv.double(), keep, p, dout.double()), R.backward(qkv, keep, p, dout)
        got = _run(qkv, dout, p)
        got["lse"] = got["lse"].double() * LN2                        # the op's log2 units -> natural
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (p, k)
        bad += _check(f"{pattern} B{B} L{L} p{p}", [(k, got[k], r64[k], r32[k]) for k in ("out", "lse", "dq", "dk", "dv")])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------- counting probes
@pytest.mark.parametrize("L", [1, 65, 129])
def test_counting_uniform_rows(built_lib, L):
    """q = k = 0, p = 0: every probability is 1 / L, so dv_j = (1 / L) sum_i dO_i for EVERY key (a dropped query row, or a clone of
    row L - 1 counted in a ragged tile, moves it by 1 / L of a term), and dq, dk are exactly 0.  dO is non-zero on three rows, so that
    the sum itself costs two roundings."""
    B = 2
    rng = np.random.default_rng(L)
    qkv = torch.zeros((B, L, 768), dtype=torch.float32)
    qkv[..., 512:] = torch.from_numpy(rng.standard_normal((B, L, 256)).astype(np.float32))
    dout = torch.zeros((B, L, 256), dtype=torch.float32)
    for i in sorted({0, L // 2, L - 1}):
        dout[:, i] = torch.from_numpy(rng.uniform(0.5, 1.5, (B, 256)).astype(np.float32))
    got = _run(qkv, dout, 0.0)
    assert float(got["dq"].abs().max()) == 0.0 and float(got["dk"].abs().max()) == 0.0
    want = (dout.double().sum(dim=1, keepdim=True) / L).expand(B, L, 256)
    ulp = torch.exp2(torch.frexp(want)[1].double() - 24.0)
    worst = float(((got["dv"].double().cpu() - want).abs() / ulp).max())
    print(f"L {L}: dv within {worst:.2f} ulp of (1 / L) sum_i dO_i")
    assert worst <= 4.0


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_one_marked_dout_row(built_lib, p):
    """dO non-zero on one row of read 1 only: dv and dk of that read get support on every key, dq on that query only, and the other
    reads get exact zeros."""
    B, L, b0, i0 = 3, 200, 1, 137
    qkv = R.make_qkv(B, L, "normal")
    dout = torch.zeros((B, L, 256), dtype=torch.float32)
    dout[b0, i0] = R.make_dout(1, 1)[0, 0]
    got = {k: v.cpu() for k, v in _run(qkv, dout, p).items()}
    kept = torch.from_numpy(R.keep_mask(SEED, B, L, p))[b0, :, i0] if p > 0 else torch.ones((8, L), dtype=torch.bool)
    dv = got["dv"][b0].reshape(L, 8, 32)
    assert torch.equal((dv != 0).all(dim=-1).T, kept)                  # every kept key of every head, and only those
    assert bool((got["dk"][b0].reshape(L, 8, 32) != 0).any(dim=-1).all())
    assert bool((got["dq"][b0, i0] != 0).all())
    rest = got["dq"].clone()
    rest[b0, i0] = 0.0
    assert float(rest.abs().max()) == 0.0
    for b in (0, 2):
        assert float(got["dqkv"][b].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------- independence, determinism
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_reads_are_independent_and_calls_repeat(built_lib, p):
    B, L = 3, 200
    qkv, dout = R.make_qkv(B, L, "normal"), R.make_dout(B, L)
    whole, again = _run(qkv, dout, p), _run(qkv, dout, p)
    alone = _run(qkv[:1], dout[:1], p)                                 # read 0 as a batch of one: the same b = 0, the same seed
    for k in ("out", "lse", "dqkv"):
        assert torch.equal(whole[k], again[k]), k                      # two identical calls: identical bits
        assert torch.equal(whole[k][:1], alone[k]), k
    if p > 0:
        other = _run(qkv, dout, p, seed=SEED + 1)
        assert not torch.equal(whole["out"], other["out"])             # (the seed counts)
        assert torch.equal(whole["lse"], other["lse"])                 # ... but l sums the undropped probabilities


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(built_lib):
    from chimeralm_amd import _native as N

    lib = _lib()
    B, L = 2, 40
    assert lib.clm_attn_train_workspace_bytes(0, 5) == N.E_INVALID and lib.clm_attn_train_workspace_bytes(1, 0) == N.E_INVALID
    assert lib.clm_attn_train_workspace_bytes(2, 65) == 4 * 2 * 8 * 65
    assert lib.clm_attn_train_workspace_bytes(1, 1) == 32              # rounded up to 16 bytes
    qkv = R.make_qkv(B, L, "normal").cuda()
    n = {"out": B * L * 256, "lse": B * 8 * L, "dout": B * L * 256, "dqkv": B * L * 768, "ws": B * 8 * L, "keep": B * 8 * L * L // 4}
    t = {k: torch.full((v + 4,), float("nan"), dtype=torch.float32, device="cuda") for k, v in n.items()}
    s = _stream()

    def fwd(qp=qkv.data_ptr(), op=t["out"].data_ptr(), lp=t["lse"].data_ptr(), b=B, l=L, p=0.1):
        return lib.clm_attn_train_forward(qp, op, lp, b, l, p, SEED, s)

    def bwd(ptrs=None, b=B, l=L, p=0.1, **kw):
        a = dict(qkv=qkv.data_ptr(), out=t["out"].data_ptr(), lse=t["lse"].data_ptr(), dout=t["dout"].data_ptr(), dqkv=t["dqkv"].data_ptr(),
                 ws=t["ws"].data_ptr())
        a.update(kw)
        return lib.clm_attn_train_backward(a["qkv"], a["out"], a["lse"], a["dout"], a["dqkv"], a["ws"], b, l, p, SEED, s)

    def mask(kp=t["keep"].data_ptr(), b=B, l=L, p=0.1):
        return lib.clm_attn_train_mask(kp, b, l, p, SEED, s)

    for call in (fwd, bwd, mask):
        for kw in (dict(b=0), dict(l=0), dict(b=-1), dict(p=-0.1), dict(p=1.0), dict(p=float("nan")), dict(b=1 << 20, l=1 << 20)):
            assert call(**kw) == N.E_INVALID, (call.__name__, kw)
    for kw in (dict(qp=qkv.data_ptr() + 4), dict(op=t["out"].data_ptr() + 4), dict(lp=t["lse"].data_ptr() + 8), dict(qp=None), dict(op=None)):
        assert fwd(**kw) == N.E_INVALID, kw
    for k in ("qkv", "out", "lse", "dout", "dqkv", "ws"):
        assert bwd(**{k: t["out"].data_ptr() + 4}) == N.E_INVALID and bwd(**{k: None}) == N.E_INVALID, k
    assert mask(kp=t["keep"].data_ptr() + 1) == N.E_INVALID and mask(kp=None) == N.E_INVALID
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool(torch.isnan(v).all()), f"a refused call wrote to {k}"
    assert fwd() == 0                                                  # (and the same arguments, unrefused, do launch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t["out"][: n["out"]]).all())
