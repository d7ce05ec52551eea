"""The 16-bit self-attention kernel (csrc/attention.hip attention_fwd_kernel<PREC, HILO>) in its three modes -- fp16, bf16 and the
two-plane HILO variant of the transformer's fp16c mode -- through `clm_attention_fwd`, held to the per-element bound of
tests/attention_reference.py: the fp64 softmax(q k^T / sqrt(32)) v of the 16-bit inputs, `max(err / tol) <= 1` with tol derived from
the number formats (no safety factor; tests/test_attention16_host.py proves it on a CPU emulation of the kernel's arithmetic).

  a. five score patterns x twelve shapes, every launch twice (bitwise equal), HILO reconstructed as (hi + lo) / 64 in fp64;
  b. every residue of the ragged last tile: L = 1 .. 130, in tile 0 and tile 1, both 32-key blocks of the mask formula;
  c. every key counted exactly once: q = k = 0 and one marked key per (read, channel) -- 1 / L where the key exists, exactly 0
     where it does not (the uniform case, which no rounding bound resolves at 4,096 keys);
  d. the HILO planes of (a): fp16(hi + lo) == hi up to the round-to-even tie, |lo| <= ulp(hi) / 2, hi = the fp16 output x 64;
  e. every launch of (a) - (c) writes into a buffer one read longer, NaN-filled: the tail (HILO: behind the second plane) stays;
  f. a stream that is not the default one gives the same bits;
  and the entry's argument checks: CLM_PREC_F16C accepted, the fp32 arithmetics and misaligned pointers refused before any launch.

Each of these five source mutations of attention.hip (memory-safe: the loads stay clamped), applied alone on a scratch copy,
against this file and against the older tests/test_gpu_attention.py::test_attention_matches_oracle_fp16.  The table is of the
kernel as it was when it had a tile loop of its own.  Mutations 1, 3 and 4 now sit in `attention_tiles`, the one loop under all
three MFMA attention kernels (the mask line, the `o[r] *= alpha` line, `ntiles`), so they would break attention32_kernel and
attention_x3_kernel too; 2 is `v_row`, shared by `A16::store_tile` and `AX3::store_tile`; 5 is the HILO branch of
attention_fwd_kernel's own output stage.  They were not run again: the kernels' outputs are bit-identical to before
(profiles/attention_tiles_ab.txt).

  mutation                               fails here (of 75)                                   worst err / tol        the older fp16 test
  1 mask `>= L` becomes `> L`            44: (a) 33, (b) 2, (c) all 9                         1,159 (L = 2, hilo)    notices: 4 of 9, 0.17 .. 0.51
  2 `v_row` is the identity              63: (a) 55, (b) 2, (c) 6 (not 17 x 4,09x: there all  1.5e7 (bf16)           notices: 8 of 9, 1.2 .. 4.0
                                         p are equal and a permutation inside a tile is void)
  3 no `o[r] *= alpha`                   38: (a) 36, (b) 2 (needs two tiles and a maximum     9.4e6 (bf16)           notices: 6 of 9, 2.4 .. 19
                                         that moves; (c) has alpha = 1 throughout)
  4 `ntiles = max(L / KT, 1)`            39: (a) 28, (b) 2, (c) all 9                         3.7e5 (bf16)           notices: 3 of 9, 0.49 .. 1.1
  5 HILO lo plane written as zeros       4: (c) the 3 hilo cases (256 .. 424 x the allowed    1.259 (L = 2, hilo)    passes: it never runs HILO
                                         2^-20), (b) `normal`; (a) stays inside (0.92)

(a) - (c) as above; "worst err / tol" is the largest ratio that (a) or (b) printed.  Mutation 5 shows what the rounding bound cannot
see: with p rounded to 11 bits the bound is u * sum w |v| wide, and a lost lo plane (2^-12 of |o|) hides inside it except at L = 2;
the counting probe, whose p are exact, resolves it 256-fold.

What the file found when it first ran (fixed in attention.hip with this file): under -ffp-contract=fast the compiler rounded the
HILO product o * sc to fp16 twice, through fp32 for the stored hi and directly from the exact product for the hi that lo was
measured against.  Where the two fell on different sides of an fp16 midpoint the stored pair was a whole ulp(hi) off -- 1 x 48
`ragged_max`, query 34, channel 201: hi = 131.0, lo = -0.0625 for 131.0625 -- about one element in 10^4: err / tol up to 1.77, above 1 on
8 of the 60 cases of (a) and at 36 of the 260 lengths of (b), fp16 and bf16 inside throughout.  After the fix the worst ratios
on an MI355X are fp16 0.71, bf16 0.83, hilo 0.78.
"""
import ctypes as C

import pytest
import torch

import attention_reference as ar
from test_gpu_attention import ATT32_PATTERNS, _qkv32

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 63), (1, 64), (3, 65), (2, 127), (1, 128), (2, 129), (3, 513), (2, 1000), (1, 4095), (1, 4096), (1, 4097)]
WORST: dict = {}                            # (mode, pattern) -> worst err / tol seen in this session, printed as the cases run


def _prec(mode: str) -> int:
    from chimeralm_amd import _native as N

    return {"fp16": N.PREC_F16, "bf16": N.PREC_BF16, "hilo": N.PREC_F16C}[mode]


def _run16(qkv: torch.Tensor, mode: str, keep_on_device: bool = False) -> torch.Tensor:
    """clm_attention_fwd on the current stream into a buffer one read longer than the output (HILO: than both planes), pre-filled
    with the type's NaN; the tail must come back untouched.  Returns [B, L, 256], or [2, B, L, 256] (hi, lo) for "hilo"."""
    from chimeralm_amd import _native as N

    assert qkv.is_cuda and qkv.is_contiguous() and qkv.dtype == ar.DTYPE[mode]
    B, L, _ = qkv.shape
    planes = 2 if mode == "hilo" else 1
    n = planes * B * L * 256
    buf = torch.full((n + L * 256,), float("nan"), dtype=qkv.dtype, device="cuda")
    guard = buf[n:].view(torch.int16).clone()
    st = torch.cuda.current_stream()
    rc = N.load().clm_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(buf.data_ptr()), B, L, _prec(mode), C.c_void_p(st.cuda_stream))
    assert rc == 0
    st.synchronize()
    assert torch.equal(buf[n:].view(torch.int16), guard), f"clm_attention_fwd ({mode}) wrote past its output"
    out = buf[:n].reshape((2, B, L, 256) if planes == 2 else (B, L, 256))
    return out if keep_on_device else out.cpu()


_REF: dict = {}


def _reference(B: int, L: int, pattern: str, mode: str):
    """(qkv 16-bit, ref, tol) of one case, computed once per operand type (fp16 and hilo share operands and reference) and kept
    for the tests that meet the same case again (~0.3 GB for the whole file)."""
    dt = ar.DTYPE[mode]
    key = (B, L, pattern, dt)
    if key not in _REF:
        qkv = ar.round_inputs(_qkv32(B, L, pattern), mode)
        _REF[key] = (qkv, *ar.reference_and_bound(qkv, "bf16" if dt == torch.bfloat16 else "fp16"))
    qkv, ref, tol = _REF[key]
    return qkv, ref, (ar.hilo_bound(ref, tol) if mode == "hilo" else tol)


def _check_case(B: int, L: int, pattern: str, twice: bool, planes: bool) -> dict:
    ratios, plain = {}, None
    for mode in ar.MODES:
        qkv, ref, tol = _reference(B, L, pattern, mode)
        dev = qkv.cuda()
        got = _run16(dev, mode)
        if twice:
            assert torch.equal(got.view(torch.int16), _run16(dev, mode).view(torch.int16)), f"{mode}: two launches differ"
        ratios[mode] = ar.worst_ratio(ar.to_float64(got, mode), ref, tol)
        WORST[(mode, pattern)] = max(WORST.get((mode, pattern), 0.0), ratios[mode])
        if mode == "fp16":
            plain = got
        if mode == "hilo" and planes:
            ar.check_hilo_planes(got[0], got[1], plain)
    return ratios


@pytest.mark.parametrize("pattern", ATT32_PATTERNS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_patterns_and_shapes_inside_the_bound(built_lib, B, L, pattern):
    """(a), (d), (e): one whole tile, ragged tiles, several query tiles, the long-context 4,096 and its neighbours."""
    ratios = _check_case(B, L, pattern, twice=True, planes=True)
    print(f"attention16 {B} x {L} {pattern}: max err / tol " + ", ".join(f"{m} {r:.3f}" for m, r in ratios.items())
          + "; worst so far " + ", ".join(f"{m} {WORST[(m, pattern)]:.3f}" for m in ar.MODES))
    for mode, r in ratios.items():
        assert r <= 1.0, f"{mode} {B} x {L} {pattern}: max |attention - fp64| / tol = {r:.3f}"


@pytest.mark.parametrize("pattern", ["normal", "ragged_max"])
def test_every_residue_of_the_last_tile(built_lib, pattern):
    """(b): L = 1 .. 130 -- all 64 residues of the mask formula in tile 0 and in tile 1."""
    worst = {m: (0.0, 0) for m in ar.MODES}
    failed = []
    for L in range(1, 131):
        for mode, r in _check_case(1, L, pattern, twice=False, planes=True).items():
            worst[mode] = max(worst[mode], (r, L))
            if not r <= 1.0:
                failed.append(f"{mode} L={L}: {r:.3g}")
    print(f"attention16 L = 1 .. 130 {pattern}: worst err / tol " + ", ".join(f"{m} {r:.3f} (L = {L})" for m, (r, L) in worst.items()))
    assert not failed, f"{pattern}: outside the bound at " + "; ".join(failed[:12]) + f" ({len(failed)} in all)"


@pytest.mark.parametrize("mode", ar.MODES)
@pytest.mark.parametrize("shapes", [[(1, L) for L in range(1, 131)], [(17, 4095), (17, 4096), (17, 4097)], [(5, 1000)]],
                         ids=["L1to130", "B17_L4095to4097", "B5_L1000"])
def test_every_key_counted_exactly_once(built_lib, shapes, mode):
    """(c): B = 17 marks all 4,097 keys (256 per read); 5 x 1,000 mixes reads, heads and query tiles under the `g & 7` mapping."""
    worst, failed = 0.0, []
    for B, L in shapes:
        qkv, marked = ar.counting_case(B, L, mode)
        assert marked.sum().item() == min(L, 256 * B)
        try:
            worst = max(worst, ar.check_counting(_run16(qkv.cuda(), mode, keep_on_device=True), marked, L, mode))
        except AssertionError as e:
            if "wrote past" in str(e):
                raise
            failed.append(str(e))
    print(f"attention16 counting {mode} {shapes[0]} .. {shapes[-1]}: worst |got - 1 / L| / allowed = {worst:.3f}")
    assert not failed, "; ".join(failed[:8]) + f" ({len(failed)} shapes in all)"


@pytest.mark.parametrize("mode", ar.MODES)
def test_another_stream_gives_the_same_bits(built_lib, mode):
    """(f): 2 x 129 `ragged_max` on a torch.cuda.Stream of its own against the default stream."""
    qkv = _reference(2, 129, "ragged_max", mode)[0].cuda()
    want = _run16(qkv, mode)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        got = _run16(qkv, mode)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_arguments_hilo_accepted_exact_modes_and_misaligned_pointers_refused(built_lib):
    from chimeralm_amd import _native as N

    lib = N.load()
    qkv = torch.zeros((2 * 3 * 768 + 64,), dtype=torch.float16, device="cuda")
    out = torch.full((2 * 2 * 3 * 256 + 64,), float("nan"), dtype=torch.float16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert qkv.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    for prec in (N.PREC_F32, N.PREC_F16X3, 5, -1):                                 # the exact arithmetics have clm_attention_exact_fwd
        assert lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), 2, 3, prec, st) == N.E_INVALID
    for prec in (N.PREC_F16, N.PREC_BF16, N.PREC_F16C):
        for dq, do in ((2, 0), (8, 0), (0, 2), (0, 4), (2, 2)):                    # bytes: qkv needs 16, out needs 8
            assert lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr() + dq), C.c_void_p(out.data_ptr() + do), 2, 3, prec, st) == N.E_INVALID
        assert lib.clm_attention_fwd(None, C.c_void_p(out.data_ptr()), 2, 3, prec, st) == N.E_INVALID
        assert lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), 0, 3, prec, st) == N.E_INVALID
        assert lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), 2, 0, prec, st) == N.E_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call launched something"
    # aligned offsets are fine: 16 bytes into qkv, 8 bytes into out; v = 0 gives an all-zero output in both planes
    assert lib.clm_attention_fwd(C.c_void_p(qkv.data_ptr() + 16), C.c_void_p(out.data_ptr() + 8), 2, 3, N.PREC_F16C, st) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[:4]).all() and (got[4: 4 + 2 * 2 * 3 * 256] == 0).all() and torch.isnan(got[4 + 2 * 2 * 3 * 256:]).all()
