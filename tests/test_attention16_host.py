"""The per-element bound of tests/attention_reference.py, proven without a GPU: a torch-CPU emulation of the 16-bit attention
kernel's arithmetic (64-key online softmax, p rounded to 16 bits, fp32 accumulation, output rounding or the two HILO planes) stays
inside it in all three modes and on all five score patterns, and the same emulation is OUTSIDE it against a reference that leaves
the last key out -- wherever the pattern gives that key weight (`first_tile_max` puts it >= 40 below the maximum by construction:
its weight is below e^-40, so a rounding bound cannot see it; the counting probe of tests/test_gpu_attention16.py covers that)."""
import pytest
import torch

import attention_reference as ar
from test_gpu_attention import ATT32_PATTERNS, _qkv32

# L = 65: one whole tile and a one-key ragged tile; 1,000: 16 tiles, ragged; 4,097 (the long-context shape + 1; `large` and `normal`
# only, which had the highest ratios: the fp64 reference of one 4,097-position read takes about a second)
CASES = [(L, p) for L in (65, 1000) for p in ATT32_PATTERNS] + [(4097, "large"), (4097, "normal")]


@pytest.mark.parametrize("L,pattern", CASES)
def test_emulation_inside_the_bound_and_a_dropped_key_outside(L, pattern):
    x = _qkv32(1, L, pattern)
    shared = {}
    for mode in ar.MODES:
        qkv = ar.round_inputs(x, mode)
        if qkv.dtype not in shared:                                                # fp16 and hilo share operands and reference
            shared[qkv.dtype] = ar.reference_and_bound(qkv, mode, with_dropped=True)
        ref, tol, dropped = shared[qkv.dtype]
        if mode == "hilo":
            tol = ar.hilo_bound(ref, tol)
        got = ar.to_float64(ar.emulate(qkv, mode), mode)
        ratio = ar.worst_ratio(got, ref, tol)
        ratio_dropped = ar.worst_ratio(got, dropped, tol)
        print(f"attention16 host {mode} 1 x {L} {pattern}: emulation max err / tol = {ratio:.3f}; against the reference without "
              f"the last key {ratio_dropped:.3g}")
        assert ratio <= 1.0, f"{mode} {L} {pattern}: the emulation is {ratio:.3f} x the derived bound"
        if pattern != "first_tile_max":
            assert ratio_dropped > 1.0, f"{mode} {L} {pattern}: a dropped key moves no element past the bound ({ratio_dropped:.3g})"


def test_hilo_planes_of_the_emulation():
    """The plane invariants that tests/test_gpu_attention16.py asks of the kernel hold for the emulation, rounding ties included."""
    qkv = ar.round_inputs(_qkv32(2, 129, "normal"), "hilo")
    hi, lo = ar.emulate(qkv, "hilo")
    ar.check_hilo_planes(hi, lo, ar.emulate(qkv, "fp16"))
    odd_ties = ((hi.float() + lo.float()).half() != hi).sum().item()
    assert 0 < odd_ties < 20                                                      # the tie is real: the bitwise identity alone is too strict
    with pytest.raises(AssertionError):
        ar.check_hilo_planes(hi, 3 * lo)


@pytest.mark.parametrize("mode", ar.MODES)
def test_counting_probe_on_the_emulation(mode):
    """Every key counted exactly once: the emulation passes, and the probe sees a clone of the last key or a dropped key."""
    for B, L in [(1, 1), (1, 63), (1, 65), (1, 130), (3, 600)]:
        qkv, marked = ar.counting_case(B, L, mode)
        assert marked.sum().item() == min(L, 256 * B)
        got = ar.emulate(qkv, mode)
        ar.check_counting(got, marked, L, mode)
        if L > 1:
            with pytest.raises(AssertionError):                                   # key L - 1 counted twice: 2 / (L + 1) where 1 / L belongs
                clone = ar.emulate(torch.cat((qkv, qkv[:, -1:]), dim=1), mode)
                ar.check_counting(clone[..., :L, :], marked, L, mode)
            with pytest.raises(AssertionError):                                   # key L - 1 dropped: its channel is 0
                ar.check_counting(ar.emulate(qkv[:, : L - 1], mode)[..., :1, :].expand(*got.shape[:-2], L, 256), marked, L, mode)
