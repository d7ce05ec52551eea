"""DNAConvNet forward throughput on one MI355X: reads/s at 256 reads x 8,193 tokens (the length of bench.py's headline batch),
exact fp32 and fp16x3.

    python tools/cnn_bench.py [--batch 256] [--tokens 8193] [--warmup 3] [--steps 20] [--precisions fp32,fp16x3]

Seeded random weights of the production shape (the module's own initialisation, BatchNorm statistics perturbed), token ids
uniform over A/C/G/T.  Each step is timed with HIP events on the launch stream; the median of the timed steps after the warm-up
is reported, one JSON line per precision.  FLOPs on the matrix cores: blocks 1 and 2 are 2 x 256 x 1792 x (L/4 + L/16) per read
(K = 7 x 256); block 0's table sums add 7 x 256 x L plus the head's 2 x 256 x 512 -- the roofline figure uses blocks 1 and 2 against
the fp32 MFMA peak (157.3 TFLOP/s; fp16x3 runs three fp16 MFMAs per product at 1/16 the cost each)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FP32_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=8193)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--precisions", default="fp32,fp16x3")
    a = ap.parse_args()
    from chimeralm_amd.cnn import DNAConvNet

    dev = torch.device("cuda", 0)
    B, L = a.batch, a.tokens
    gemm = 2 * 256 * 1792 * (L // 4 + L // 16)
    table = 7 * 256 * L
    head = 2 * 256 * 512 + 2 * 512 * 2
    print(f"FLOP per read: blocks 1 + 2 {gemm / 1e9:.3f} G (2 x 256 x 1792 x (L/4 + L/16)), block 0 table sums {table / 1e6:.1f} M, "
          f"head {head / 1e6:.2f} M", flush=True)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(7, 11, (B, L), generator=g, dtype=torch.int64).to(dev)
    for prec in a.precisions.split(","):
        torch.manual_seed(0)
        net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7],
                         pool_sizes=[4, 4, 4], hidden_dim=512, number_of_classes=2, precision=prec)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.normal_(0.0, 0.2, generator=g)
                    m.running_var.uniform_(0.5, 2.0, generator=g)
        st = torch.cuda.current_stream(dev)
        for _ in range(a.warmup):
            net(ids)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            out = net(ids)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert torch.isfinite(out).all()
        med = statistics.median(ms)
        res = {"net": "DNAConvNet", "precision": prec, "batch": B, "tokens": L, "median_ms": round(med, 3),
               "min_ms": round(min(ms), 3), "reads_per_s": round(B / (med / 1e3), 1), "steps": a.steps,
               "gemm_gflop_per_read": round(gemm / 1e9, 4),
               "gemm_tflops_if_all_time": round(B * gemm / (med / 1e3) / 1e12, 1),
               "fp32_peak_fraction_if_all_time": round(B * gemm / (med / 1e3) / FP32_PEAK, 3)}
        print(json.dumps(res), flush=True)
        net.close()


if __name__ == "__main__":
    main()
