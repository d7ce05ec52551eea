"""Child process of tests/test_gpu_h_order.py: the fused 16-bit forwards of its cases under ONE setting of CLM_DEBUG (read when a
handle is created, so each setting gets a process of its own), results as an .npz:   python tests/h_order_child.py OUT.npz"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from chimeralm_amd.engine import Engine  # noqa: E402
from oracle import hyena_oracle as ho  # noqa: E402

# (precision, B, L): two whole tiles + the peeled token and an odd batch; no peel; three tiles; a partial last tile (row order)
CASES = [("fp16c", 3, 257), ("fp16c", 2, 256), ("fp16c", 2, 385), ("fp16c", 2, 300), ("fp16", 3, 257)]
PAD_CASE = ("fp16c", 2, 513, 300)          # read 0 starts with 300 [PAD]: its tile 0 is in no launch's list


def case_ids(B, L, pads=0):
    ids, _ = ho.synthetic_batch(5, B, L - 1, seed=99)
    if pads:
        ids[0, :pads] = 4
    return ids


def main(out_path: str) -> None:
    sd = ho.make_state_dict(0, head_scale=3.0)
    engines = {}
    for prec in ("fp16c", "fp16", "fp32"):
        e = Engine("cuda:0", precision=prec, chunk_reads=4)
        e.load_state_dict(sd)
        if prec == "fp16c":
            e.set_f16c_min_len(1)                      # the 16-bit kernels of the mode at every length
        engines[prec] = e
    out = {}
    for prec, B, L in CASES:
        t = torch.from_numpy(case_ids(B, L)).cuda()
        assert engines[prec].effective_precision(L) == prec
        out[f"logits_{prec}_{B}x{L}"] = engines[prec].forward(t).cpu().numpy()
        if L == 257:                                   # what the last storing block left, straight after the complete forward
            out[f"h_{prec}_{B}x{L}"] = engines[prec].debug_fetch("h", (B, L, 256))
        out[f"exact_{prec}_{B}x{L}"] = engines["fp32"].forward(t).cpu().numpy()
    prec, B, L, pads = PAD_CASE
    out["logits_pad"] = engines[prec].forward(torch.from_numpy(case_ids(B, L, pads)).cuda()).cpu().numpy()
    np.savez(out_path, **out)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main(sys.argv[1])
