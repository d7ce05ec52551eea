"""Mamba nets' forward throughput on one MI355X: reads/s for `mamba` and `mambasp`, exact fp32 and fp16x3, at 256 reads x 8,193
tokens (the length of bench.py's headline batch) and at the long-read shapes 4 x 30,000 (`mamba`, its model_max_length) and
4 x 32,769 (`mambasp`).

    python tools/mamba_bench.py [--nets mamba,mambasp] [--precisions fp32,fp16x3] [--shapes big,long] [--warmup 2] [--steps 5]
                                [--trajectory-stride 128]

`--trajectory-stride S`: every forward also makes the running-verdict request (csrc/mamba_verdict.hip), for its cost against a run
without.

Seeded random weights of the reference configs (the modules' own initialisation: mamba_ssm's A / dt / D ranges), token ids uniform
over A/C/G/T.  Each step is timed with HIP events on the launch stream; the median of the timed steps after the warm-up is
reported, one JSON line per (net, precision, shape).  FLOPs per token and layer: in_proj 2 d (2 di + 2 N + H), out_proj 2 di d (the
projections, on the matrix cores), and the scan's products, about 2 H (Q N + Q P + 2 N P) at chunk Q = 64 (on the VALU).  The
roofline figure divides the projections' FLOPs by the whole step's time against the fp32 MFMA peak (157.3 TFLOP/s), so it is a
lower bound of the projection kernels' own fraction; a `rocprofv3 --kernel-trace --stats` run gives the split."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FP32_PEAK = 157.3e12
CFG = {"mamba": dict(d=256, layers=12, N=16, expand=2), "mambasp": dict(d=512, layers=3, N=128, expand=3)}
SHAPES = {"big": {"mamba": (256, 8193), "mambasp": (256, 8193)}, "long": {"mamba": (4, 30000), "mambasp": (4, 32769)}}


def flops_per_token(net: str) -> tuple[float, float]:
    c = CFG[net]
    d, N = c["d"], c["N"]
    di = c["expand"] * d
    H = di // 64
    proj = 2 * d * (2 * di + 2 * N + H) + 2 * di * d
    scan = 2 * H * (64 * N + 64 * 64 + 2 * N * 64)
    return proj * c["layers"], scan * c["layers"]


def make(net: str, prec: str):
    from chimeralm_amd import mamba

    c = CFG[net]
    torch.manual_seed(0)
    if net == "mamba":
        return mamba.MambaSequenceClassification(vocab_size=12, embedding_dim=c["d"], number_of_layers=c["layers"], model_max_length=30000,
                                                 dropout=0.1, number_of_classes=2, d_state=c["N"], expand=c["expand"], precision=prec)
    return mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=c["d"], number_of_layers=c["layers"], number_of_classes=2,
                                               dropout=0.2, d_state=c["N"], expand=c["expand"], precision=prec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="mamba,mambasp")
    ap.add_argument("--precisions", default="fp32,fp16x3")
    ap.add_argument("--shapes", default="big,long")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--trajectory-stride", type=int, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for netname in a.nets.split(","):
        proj, scan = flops_per_token(netname)
        print(f"{netname}: FLOP per token, all layers: projections {proj / 1e6:.2f} M, scan {scan / 1e6:.2f} M", flush=True)
        for prec in a.precisions.split(","):
            net = make(netname, prec)
            if a.trajectory_stride is not None:
                from chimeralm_amd.engine import check_trajectory_stride

                net.trajectory_stride = check_trajectory_stride(a.trajectory_stride)
            for shape in a.shapes.split(","):
                B, L = SHAPES[shape][netname]
                ids = torch.randint(7, 11, (B, L), generator=g, dtype=torch.int64).to(dev)
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
                tok = B * L
                res = {"net": netname, "precision": prec, "batch": B, "tokens": L, "median_ms": round(med, 2), "min_ms": round(min(ms), 2),
                       "reads_per_s": round(B / (med / 1e3), 2), "steps": a.steps, "trajectory_stride": a.trajectory_stride,
                       "proj_tflops_if_all_time": round(tok * proj / (med / 1e3) / 1e12, 1),
                       "fp32_peak_fraction_if_all_time": round(tok * proj / (med / 1e3) / FP32_PEAK, 3)}
                print(json.dumps(res), flush=True)
            net.close()


if __name__ == "__main__":
    main()
