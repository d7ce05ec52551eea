"""What a training step of DNAConvNet costs on one MI355X, part by part (chimeralm_amd/cnntrain.py, csrc/cnn_train.hip).

    python tools/cnn_train_bench.py [--shapes 8x8193,8x32769] [--warmup 5] [--steps 50] [--dropout 0.1] [-o FILE]
    rocprofv3 --output-format csv --kernel-trace --stats -d DIR -- python tools/cnn_train_bench.py --shapes 8x8193 --steps 10     (a run of its own)
    python tools/cnn_train_bench.py --kernel-stats DIR/.../*_kernel_stats.csv --shapes 8x8193 [-o FILE]        (no GPU needed)

Seeded weights of the module's own initialisation, token ids uniform over A/C/G/T.  The first form times, with device events on the
launch stream (median of the timed steps after the warm-up): the whole step (zero_grad, forward, loss, backward, Adam), the engine's
training forward (clm_cnn_train_forward: pack, table, three blocks, mean), its backward (clm_cnn_train_backward), fc + loss forward
and backward in torch, the optimizer -- and, as the yardstick, the exact-fp32 INFERENCE forward of the same batch in the same call.
The backward does two GEMMs per block where the forward does one, so a step near 3 x that forward plus the BatchNorm passes' memory
traffic is the expectation; the line says what was measured.  One line per shape, also appended to FILE (profiles/cnn_train_bench.txt
is one).

Kernel times come from rocprofv3 in a run of its own (tracing slows the host); the third form reads its kernel statistics and prints
the mean time per launch of every cnn_train_* kernel, and for the three matrix-core kernels the rate over that time against the fp32
MFMA peak of 157.3 TFLOP/s: forward GEMM, dx GEMM and dW each do 2 x 256 x 1,792 FLOP per position of blocks 1 and 2."""
from __future__ import annotations

import argparse
import csv
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FP32_PEAK = 157.3e12
CFG = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4], hidden_dim=512,
           number_of_classes=2, padding_idx=4)


def gemm_flop(B: int, L: int) -> int:
    """FLOP of one implicit GEMM pass over blocks 1 and 2 (forward, dx or dW): 2 x 256 x 7 x 256 per position."""
    return 2 * 256 * 7 * 256 * B * (L // 4 + L // 16)


def kernel_stats(path: str, shapes, out):
    rows = list(csv.DictReader(open(path)))
    name_col = next(c for c in rows[0] if c.lower() in ("name", "kernelname", "kernel_name"))
    calls_col = next(c for c in rows[0] if c.lower() == "calls")
    total_col = next(c for c in rows[0] if c.lower().startswith("totalduration"))
    lines = []
    for r in rows:
        n = r[name_col]
        if "cnn_train_" not in n:
            continue
        short = n.split("cnn_train_", 1)[1].split("(")[0].split("<")[0]
        calls, total_ms = int(r[calls_col]), float(r[total_col]) / 1e6
        line = f"cnn_train_{short}: {calls} launches, mean {total_ms / calls * 1e3:.1f} us, total {total_ms:.3f} ms"
        if len(shapes) == 1 and short in ("gemm7_kernel", "dw_kernel"):
            B, L = shapes[0]
            rate = gemm_flop(B, L) * (calls / 2) / (total_ms / 1e3)   # every two launches (block 1, block 2) are one pass
            line += f" | {rate / 1e12:.1f} TFLOP/s, {rate / FP32_PEAK:.2f} of the fp32 MFMA peak ({B} x {L})"
        lines.append(line)
    out("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x8193,8x32769")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("-o", "--output", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]

    def out(text):
        print(text, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(text + "\n")

    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, shapes, out)

    import torch
    import torch.nn.functional as F

    from chimeralm_amd import cnntrain
    from chimeralm_amd.cnn import DNAConvNet

    dev = torch.device("cuda", 0)

    def timed(fn):
        st = torch.cuda.current_stream(dev)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    torch.manual_seed(0)
    net = DNAConvNet(**CFG, dropout=a.dropout, precision="fp32", trainable=True).to(dev)
    infer = DNAConvNet(**CFG, precision="fp32").to(dev).eval()
    infer.load_state_dict(net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    for B, L in shapes:
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(7, 11, (B, L), generator=g, dtype=torch.int64).to(dev)
        labels = (torch.arange(B) % 2).to(dev)
        with torch.no_grad():
            t_inf = timed(lambda: infer(ids))
        net.train()

        def step():
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(net(ids), labels).backward()
            opt.step()

        t_step = timed(step)
        eng = net.train_engine(dev)
        params = [p.detach() for p in cnntrain.engine_parameters(net)]
        Ls = cnntrain.block_lengths(L)
        keeps = [(torch.rand((B, Ls[i + 1], 256), device=dev) >= a.dropout).to(torch.uint8) for i in range(3)] if a.dropout > 0 else None
        scale = 1.0 / (1.0 - a.dropout)
        t_fwd = timed(lambda: eng.forward(ids, params, keeps, scale))
        dp = torch.randn(B, 256, generator=g).to(dev)

        def fwd_bwd():
            gen = eng.forward(ids, params, keeps, scale)[3]
            eng.backward(gen, dp, params)

        t_bwd = timed(fwd_bwd) - t_fwd
        pooled = eng.forward(ids, params, keeps, scale)[0]

        def fc():
            x = pooled.detach().requires_grad_(True)
            F.cross_entropy(net.fc(x), labels).backward()

        t_fc = timed(fc)
        t_opt = timed(opt.step)
        flop = gemm_flop(B, L)
        out(f"{B} x {L} dropout {a.dropout:g}: whole step {t_step:.3f} ms ({B / t_step * 1e3:.0f} reads/s) | engine forward {t_fwd:.3f} ms | engine backward "
            f"{t_bwd:.3f} ms (forward + backward timed together, less the forward) | fc fwd+bwd in torch {t_fc:.3f} ms | Adam {t_opt:.3f} ms | "
            f"fp32 inference forward {t_inf:.3f} ms: step = {t_step / t_inf:.2f} x, engine forward + backward = {(t_fwd + t_bwd) / t_inf:.2f} x | "
            f"matrix-core FLOP of the step (3 GEMM passes over blocks 1 and 2) {3 * flop / 1e9:.1f} G: {3 * flop / ((t_fwd + t_bwd) / 1e3) / 1e12:.1f} "
            f"TFLOP/s over the engine's forward + backward, {3 * flop / ((t_fwd + t_bwd) / 1e3) / FP32_PEAK:.2f} of the fp32 MFMA peak "
            f"(an end-to-end rate, not a kernel's) | workspace {eng.lib.clm_cnn_train_workspace_bytes(B, L) / 2**20:.0f} MiB")


if __name__ == "__main__":
    main()
