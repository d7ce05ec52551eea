"""Generate tests/golden/cnn_golden.npz from the reference's own `DNAConvNet` (models/components/cnn.py).

Run ONLY in the build container (needs /root/reference):   python tests/golden/make_cnn_golden.py
The reference module is loaded by file path, as make_golden.py does; nothing of it is copied.  Weights are regenerated from the
seed by tests/cnn_reference.make_cnn_state_dict, so only ids and outputs are stored: per case `{name}_ids` (int64 [B, L]),
`{name}_logits` ([B, 2], the reference module in eval mode, fp32 on the CPU), `{name}_pooled` ([B, 256], the input of `fc`) and
`{name}_meta` = (seed, B, L, pads).
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.path.insert(0, str(HERE.parent))

import cnn_reference as cr  # noqa: E402

# (name, seed, B, L, left pads): the 64-token minimum, one past it, a padded read, and the lengths of the benchmark
CASES = [("l64", 0, 2, 64, 0), ("l65", 1, 3, 65, 0), ("l777pad", 2, 3, 777, 40), ("l4101", 3, 2, 4101, 7), ("l8193", 4, 2, 8193, 0)]


def main():
    spec = importlib.util.spec_from_file_location("ref_cnn", REF / "chimeralm/models/components/cnn.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, seed, B, L, pads in CASES:
        net = mod.DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7],
                             pool_sizes=[4, 4, 4], hidden_dim=512, number_of_classes=2, dropout=0.1).eval()
        net.load_state_dict(cr.make_cnn_state_dict(seed), strict=True)
        ids = cr.synthetic_ids(100 + seed, B, L, pads)
        pooled = {}
        net.fc.register_forward_hook(lambda m, inp, o: pooled.__setitem__("v", inp[0].detach().clone()))
        with torch.no_grad():
            logits = net(torch.from_numpy(ids))
        out[f"{name}_ids"] = ids
        out[f"{name}_logits"] = logits.numpy()
        out[f"{name}_pooled"] = pooled["v"].numpy()
        out[f"{name}_meta"] = np.array([seed, B, L, pads], dtype=np.int64)
    np.savez_compressed(HERE / "cnn_golden.npz", **out)
    print("cnn_golden.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
