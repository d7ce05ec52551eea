"""Cost of the mutagenesis scan on one MI355X: the scan's mutants/s on one read against the same net's bare forward reads/s.

    python tools/explain_bench.py [--nets hyena,mambasp] [--bases 8192] [--batch 256] [--window 1] [--stride 1] [--rounds 7]
                                  [--bare-steps 4]

A scan round is `explain.position_importance` on one seeded read of `--bases` bases (mutants built on the device, the net's forward
per batch, the scores kernel behind it, the reduce kernel at the end); a bare round is `--bare-steps` forwards of the same net on
`--batch` x (bases + 1) random ids that already lie on the device -- existing code, the most the scan could reach.  Both in one
process, rounds interleaved (scan, bare, scan, ...), a host clock around work that ends in a synchronise, one warm-up round each.
Hyena runs in fp16x3 (the `explain` command's default), `mambasp` in its default fp16x3.  Seeded random weights.  One JSON line per
net: medians, the spread (min ... max) of both, and the scan's rate as a fraction of the bare forward's."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make(name: str):
    torch.manual_seed(0)
    if name == "hyena":
        from chimeralm_amd import lm

        return lm.ChimeraLM.new(precision="fp16x3", selfcheck=False).net
    if name == "mambasp":
        from chimeralm_amd import mamba

        return mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=512, number_of_layers=3, number_of_classes=2, dropout=0.2,
                                                   d_state=128, expand=3, precision="fp16x3")
    raise SystemExit(f"unknown net {name!r} (hyena, mambasp)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="hyena,mambasp")
    ap.add_argument("--bases", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bare-steps", type=int, default=4)
    a = ap.parse_args()
    from chimeralm_amd.explain import position_importance

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    read = torch.from_numpy(np.concatenate([7 + rng.integers(0, 4, size=a.bases), [1]]).astype(np.uint8))
    bare_ids = torch.from_numpy((7 + rng.integers(0, 4, size=(a.batch, a.bases + 1))).astype(np.uint8))
    bare_ids[:, -1] = 1
    bare_ids = bare_ids.to(dev)
    for name in a.nets.split(","):
        net = make(name)

        def scan():
            t = time.perf_counter()
            imp = position_importance(net, read, window=a.window, stride=a.stride, score="gap", batch_size=a.batch, device=dev)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t, imp

        def bare():
            t = time.perf_counter()
            for _ in range(a.bare_steps):
                out = net(bare_ids, None)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t, out

        scan(), bare()                                         # warm-up: workspaces, LDS attributes, the allocator's blocks
        ts, tb = [], []
        for _ in range(a.rounds):
            dt, imp = scan()
            ts.append(dt)
            dt, out = bare()
            tb.append(dt)
        assert torch.isfinite(out).all() and int(imp.n_nonfinite.item()) == 0
        rows = imp.logits.shape[0]                             # mutants + the read itself
        rs = sorted(rows / t for t in ts)
        rb = sorted(a.bare_steps * a.batch / t for t in tb)
        res = {"net": name, "bases": a.bases, "batch": a.batch, "window": a.window, "stride": a.stride, "rows_per_scan": rows,
               "rounds": a.rounds, "scan_rows_per_s": {"median": round(statistics.median(rs), 2), "min": round(rs[0], 2), "max": round(rs[-1], 2)},
               "bare_reads_per_s": {"median": round(statistics.median(rb), 2), "min": round(rb[0], 2), "max": round(rb[-1], 2)},
               "scan_over_bare": round(statistics.median(rs) / statistics.median(rb), 4),
               "scan_round_s": round(statistics.median(ts), 3), "bare_round_s": round(statistics.median(tb), 3)}
        print(json.dumps(res), flush=True)
        (net.close if hasattr(net, "close") else net._engine.close)()


if __name__ == "__main__":
    main()
