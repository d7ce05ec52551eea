"""Generate tests/golden/cnn_train_golden.npz from the reference's own `DNAConvNet` (models/components/cnn.py) in `train()`.

Run ONLY in the build container (needs /root/reference):   python tests/golden/make_cnn_train_golden.py
The reference module is loaded by file path, as make_cnn_golden.py does; nothing of it is copied.  One training step per case --
`dropout=0.0`, fp32 on the CPU, mean cross-entropy against tests/cnn_train_reference.synthetic_labels, `backward()` -- on weights from
tests/cnn_reference.make_cnn_state_dict(seed) and ids from synthetic_ids(seed, B, L, pads), so only results are stored.  Per case
`{name}_meta` = (seed, B, L, pads), `{name}_loss`, `{name}_logits`; the embedding, bias and BatchNorm gradients in full as
`{name}_g:{key}`; of each conv weight gradient taps 0, 3 and 6 of its first 8 output channels (`{name}_gs:{key}` [8, 256, 3]) and the
tensor's max-abs (`{name}_gmax:{key}`); the running statistics after the step as `{name}_r:{key}`.
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
import cnn_train_reference as ctr  # noqa: E402

# (name, seed, B, L, left pads): one tile, positions past 4 L_out, a pad prefix with L_1 = 50 and L_2 = 12, several tiles per read
CASES = [("l64", 0, 2, 64, 0), ("l67", 1, 3, 67, 0), ("l203pad", 2, 3, 203, 17), ("l1031pad", 3, 4, 1031, 100)]
TAPS = [0, 3, 6]


def main():
    spec = importlib.util.spec_from_file_location("ref_cnn", REF / "chimeralm/models/components/cnn.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, seed, B, L, pads in CASES:
        net = mod.DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7],
                             pool_sizes=[4, 4, 4], hidden_dim=512, number_of_classes=2, dropout=0.0).train()
        net.load_state_dict(cr.make_cnn_state_dict(seed), strict=True)
        ids, labels = cr.synthetic_ids(seed, B, L, pads), ctr.synthetic_labels(seed, B)
        logits = net(torch.from_numpy(ids))
        loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(labels))
        loss.backward()
        out[f"{name}_meta"] = np.array([seed, B, L, pads], dtype=np.int64)
        out[f"{name}_loss"] = loss.detach().numpy()
        out[f"{name}_logits"] = logits.detach().numpy()
        for k, p in net.named_parameters():
            g = p.grad.numpy()
            if g.ndim == 3:
                out[f"{name}_gs:{k}"] = g[:8][:, :, TAPS].copy()
                out[f"{name}_gmax:{k}"] = np.abs(g).max()
            elif k.startswith(("embedding", "conv_blocks")) or g.ndim == 1:
                out[f"{name}_g:{k}"] = g
        for k, v in net.named_buffers():
            out[f"{name}_r:{k}"] = v.numpy()
    np.savez_compressed(HERE / "cnn_train_golden.npz", **out)
    print("cnn_train_golden.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
