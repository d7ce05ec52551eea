"""Compiler-side guard of the Hyena training kernels (csrc/hyena_train.hip), as tests/test_attn_train_resources.py holds the
attention ones (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch -- a spill inside a Stockham pass is vector-memory
traffic between its LDS loads and stores --, every transform size present, and the registers that keep two waves per SIMD (one
workgroup of 512 threads per CU at 16384 points)."""
import re

from chimeralm_amd import build as B

LOGNS = range(8, 15)
TRANSFORM_KERNELS = ("hyena_train_spectrum_kernel", "hyena_train_fwd_kernel", "hyena_train_bwd_kernel")
PLAIN_KERNELS = ("hyena_train_twiddle_kernel", "hyena_train_reduce_kernel")


def _resources():
    B.build()
    out, name = {}, None
    for ln in B.RESOURCES.read_text().splitlines():
        if ln.startswith("Function Name: "):
            name = ln.split(": ", 1)[1].strip()
            out[name] = {}
        elif name and ":" in ln:
            k, v = ln.strip().split(":", 1)
            out[name][k.strip()] = v.strip()
    return {n: r for n, r in out.items() if "hyena_train_" in n}


def test_hyena_train_kernels_have_no_scratch():
    res = _resources()
    assert len(res) == len(TRANSFORM_KERNELS) * len(LOGNS) + len(PLAIN_KERNELS), sorted(res)
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, f"{name}: {r['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert r["Dynamic Stack"] == "False", name
        assert int(r["VGPRs"]) + int(r["AGPRs"]) <= 256 and int(r["Occupancy [waves/SIMD]"]) >= 2, name


def test_every_transform_size_is_instantiated():
    res = _resources()
    for kern in TRANSFORM_KERNELS:
        for logn in LOGNS:
            assert any(re.search(rf"{kern}ILi{logn}E", n) for n in res), (kern, logn)
    for kern in PLAIN_KERNELS:
        assert sum(kern in n for n in res) == 1, kern


def test_the_inference_convolution_is_untouched():
    """The new kernels carry none of the names tests/test_kernel_resources.py matches by substring."""
    for name in _resources():
        assert not any(s in name for s in ("hyena_conv_kernel", "hyena_conv_pers_kernel", "hyena_conv_seg_kernel")), name
