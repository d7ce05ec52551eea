"""Compiler-side guard of the segmented Hyena training kernels (csrc/hyena_longtrain.hip), in the pattern of
tests/test_hyena_train_resources.py (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch, no dynamic stack, the registers that
keep two waves per SIMD (one workgroup of 512 threads per CU at 147,968 B of dynamic LDS), and names that none of the other
resource tests match by substring."""
from chimeralm_amd import build as B

KERNELS = ("hyena_longtrain_twiddle_kernel", "hyena_longtrain_spectrum_kernel", "hyena_longtrain_fwd_kernel",
           "hyena_longtrain_bwd_kernel", "hyena_longtrain_reduce_kernel")
OTHERS = ("hyena_train_", "hyena_conv_kernel", "hyena_conv_pers_kernel", "hyena_conv_seg_kernel")


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
    return {n: r for n, r in out.items() if "hyena_longtrain_" in n}


def test_hyena_longtrain_kernels_have_no_scratch():
    res = _resources()
    assert len(res) == len(KERNELS), sorted(res)
    for kern in KERNELS:
        assert sum(kern in n for n in res) == 1, kern
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, f"{name}: {r['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert r["Dynamic Stack"] == "False", name
        assert int(r["VGPRs"]) + int(r["AGPRs"]) <= 256 and int(r["Occupancy [waves/SIMD]"]) >= 2, name


def test_the_other_kernels_names_are_untouched():
    """tests/test_hyena_train_resources.py counts every name with `hyena_train_`; tests/test_kernel_resources.py matches the three
    inference convolutions by substring."""
    for name in _resources():
        assert not any(s in name for s in OTHERS), name
