"""Compiler-side guard of the training attention kernels (csrc/attention_train.hip), as tests/test_kernel_resources.py holds the
inference kernels (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch -- a spill inside the tile loops is vector-memory
traffic behind the staged loads -- the occupancy the tiles were laid out for, and every variant present."""
import re

from chimeralm_amd import build as B

# kernel -> (variants, waves per SIMD at least): the forward keeps attention32_kernel's four; the two backward passes hold two more
# accumulators and both operand fragments, and their 36 KiB of LDS allow four workgroups per CU at most
KERNELS = {r"attn_train_fwd_kernel": (2, 4), r"attn_train_dq_kernel": (2, 2), r"attn_train_dkv_kernel": (2, 2),
           r"attn_train_delta_kernel": (1, 4), r"attn_train_mask_kernel": (1, 4)}


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
    return out


def test_training_attention_kernels_have_no_scratch():
    res = _resources()
    for pattern, (count, waves) in KERNELS.items():
        hits = {n: r for n, r in res.items() if re.search(pattern, n)}
        assert len(hits) == count, f"{pattern}: {sorted(hits)}"
        for name, r in hits.items():
            assert int(r["ScratchSize [bytes/lane]"]) == 0, f"{name}: {r['ScratchSize [bytes/lane]']} bytes of scratch per lane"
            assert r["Dynamic Stack"] == "False", name
            assert int(r["Occupancy [waves/SIMD]"]) >= waves, f"{name}: {r['Occupancy [waves/SIMD]']} waves per SIMD (floor {waves})"


def test_forward_without_dropout_is_the_inference_kernel_in_registers():
    """The p = 0 forward is attention_tiles<A32> with the empty hook: attention32_kernel's LDS, and its registers up to the handful
    the lse store takes."""
    res = _resources()
    inf = next(r for n, r in res.items() if "attention32_kernel" in n)
    trn = next(r for n, r in res.items() if re.search(r"attn_train_fwd_kernelILb0E", n))
    assert trn["LDS Size [bytes/block]"] == inf["LDS Size [bytes/block]"]
    assert int(trn["VGPRs"]) <= int(inf["VGPRs"]) + 8 and int(trn["AGPRs"]) == int(inf["AGPRs"])
