"""Generate tests/golden/mamba_golden.npz from the reference's own `MambaSequenceClassification` and
`MambaSequenceClassificationSP` (models/components/mamba.py).

Run ONLY in the build container (needs /root/reference):   python tests/golden/make_mamba_golden.py
The reference module is loaded by file path, as make_cnn_golden.py does; nothing of it is copied.  `mamba_ssm` (CUDA / Triton) is not
installed here, so a stand-in `mamba_ssm` module goes into sys.modules first: its `Mamba2` is tests/mamba_reference.Mamba2Ref, the
parameter container plus the sequential fp64 recurrence.  Everything around the layers -- embedding, positional term, input block,
masks, residuals, mean + max pooling, pooler, classifier and the state_dict layout -- is the reference's code.
Weights are regenerated from the seed by tests/mamba_reference.make_mamba_state_dict, so per case only `{name}_ids` (int64 [B, L]),
`{name}_mask` (fp32 [B, L], all ones when the case passes none), `{name}_logits` ([B, 2], fp64), `{name}_pooled` ([B, d], the
pooler's input) and `{name}_meta` = (variant 0 mamba / 1 mambasp, seed, B, L, pads, d_state, masked) are stored, plus `{variant}_keys` /
`{variant}_shapes`: the reference module's state_dict keys and their shapes (padded with -1 to rank 3).
"""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.path.insert(0, str(HERE.parent))

import mamba_reference as mr  # noqa: E402

# (name, variant, seed, B, L, left pads, d_state, masked): the chunk edges 63 / 64 / 65, one token, a padded read, the lengths of
# the benchmark, the masked `mamba` path and both `mamba` state sizes of the reference's configs (16: model, 64: experiment)
CASES = [("m_l1", "mamba", 0, 2, 1, 0, 16, False), ("m_l63", "mamba", 1, 2, 63, 0, 16, False), ("m_l64", "mamba", 2, 2, 64, 0, 16, False),
         ("m_l65", "mamba", 3, 2, 65, 0, 16, False), ("m_l777pad", "mamba", 4, 2, 777, 40, 16, False),
         ("m_l4101", "mamba", 5, 1, 4101, 7, 16, False), ("m_l8193", "mamba", 6, 1, 8193, 0, 16, False),
         ("m_mask", "mamba", 7, 2, 300, 0, 16, True), ("m_ds64", "mamba", 8, 2, 300, 0, 64, False),
         ("s_l1", "mambasp", 10, 2, 1, 0, 128, False), ("s_l63", "mambasp", 11, 2, 63, 0, 128, False),
         ("s_l64", "mambasp", 12, 2, 64, 0, 128, False), ("s_l65", "mambasp", 13, 2, 65, 0, 128, False),
         ("s_l777pad", "mambasp", 14, 2, 777, 40, 128, False), ("s_l4101", "mambasp", 15, 1, 4101, 7, 128, False),
         ("s_l8193", "mambasp", 16, 1, 8193, 0, 128, False)]


def case_mask(seed: int, B: int, L: int) -> np.ndarray:
    """fp32 [B, L]: ones, a zeroed stretch in the middle of read 0, the last quarter of read 1 zeroed, a few fractional values."""
    rng = np.random.default_rng(seed)
    m = np.ones((B, L), dtype=np.float32)
    m[0, L // 3:L // 3 + 40] = 0.0
    if B > 1:
        m[1, 3 * L // 4:] = 0.0
    idx = rng.integers(0, L, size=10)
    m[0, idx] = rng.uniform(0.2, 0.9, size=10).astype(np.float32)
    return m


def build_net(mod, variant: str, d_state: int):
    d, nl, _, expand, mml = mr.VARIANTS[variant]
    if variant == "mamba":
        return mod.MambaSequenceClassification(vocab_size=12, embedding_dim=d, number_of_layers=nl, model_max_length=mml, dropout=0.1,
                                               number_of_classes=2, d_state=d_state, d_conv=4, expand=expand)
    return mod.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=d, number_of_layers=nl, number_of_classes=2, dropout=0.2,
                                             headdim=64, d_state=d_state, d_conv=4, expand=expand)


def main():
    stand_in = types.ModuleType("mamba_ssm")
    stand_in.Mamba2 = mr.Mamba2Ref
    sys.modules["mamba_ssm"] = stand_in
    spec = importlib.util.spec_from_file_location("ref_mamba", REF / "chimeralm/models/components/mamba.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for variant in ("mamba", "mambasp"):
        sd = build_net(mod, variant, mr.VARIANTS[variant][2]).state_dict()
        out[f"{variant}_keys"] = np.array(list(sd.keys()))
        out[f"{variant}_shapes"] = np.array([list(v.shape) + [-1] * (3 - v.dim()) for v in sd.values()], dtype=np.int64)
    for name, variant, seed, B, L, pads, d_state, masked in CASES:
        net = build_net(mod, variant, d_state).eval()
        net.load_state_dict(mr.make_mamba_state_dict(variant, seed, d_state=d_state), strict=True)
        net = net.double()                                     # the reference's code in fp64 end to end
        ids = mr.synthetic_ids(100 + seed, B, L, pads)
        mask = case_mask(200 + seed, B, L) if masked else np.ones((B, L), dtype=np.float32)
        pooled = {}
        net.pooler.register_forward_hook(lambda m, inp, o: pooled.__setitem__("v", inp[0].detach().clone()))
        with torch.no_grad():
            logits = net(torch.from_numpy(ids), torch.from_numpy(mask).double() if masked else None)
        out[f"{name}_ids"] = ids
        out[f"{name}_mask"] = mask
        out[f"{name}_logits"] = logits.numpy()
        out[f"{name}_pooled"] = pooled["v"].numpy()
        out[f"{name}_meta"] = np.array([0 if variant == "mamba" else 1, seed, B, L, pads, d_state, int(masked)], dtype=np.int64)
        print(name, logits.numpy().round(3).tolist(), flush=True)
    np.savez_compressed(HERE / "mamba_golden.npz", **out)
    print("mamba_golden.npz", (HERE / "mamba_golden.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
