"""What a training step of SequenceCNNTransformer costs on one MI355X, with the attention core on the engine and in torch
(chimeralm_amd/tftrain.py, csrc/attention_train.hip).

    python tools/tf_train_bench.py [--cases 8x8193,4x32769] [--layers 12] [--dropout 0.1] [--warmup 3] [--steps 20] [-o FILE]

The net in its config size (configs/model/transformer.yaml), the module's own seeded initialisation, token ids uniform over A/C/G/T.
Timed with device events on the launch stream.  The two cores run in the same job on the same weights, ALTERNATING step by step
(engine, torch, engine, ...), so that clocks and neighbours move both alike; reported per core: the median of the timed steps and
their spread (min .. max).  A step is zero_grad, forward, loss, backward; no optimizer.  Then, on one layer's tensors: the core
forward (clm_attn_train_forward) and backward (clm_attn_train_backward) of the engine and of torch's
F.scaled_dot_product_attention, and the exact-fp32 INFERENCE forward of the same batch.  Live bytes: torch's peak allocation over
one step of each core (the engine's scratch is a torch tensor, so it is counted).  One line per case, also appended to FILE
(profiles/tf_train_bench.txt is one)."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x8193,4x32769")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("-o", "--output")
    a = ap.parse_args()

    def out(line):
        print(line, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(line + "\n")

    import torch

    from chimeralm_amd import tftrain
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.transformer import SequenceCNNTransformer

    dev = torch.device("cuda", 0)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        return [event_ms(fn) for _ in range(steps)]

    def fmt(ts):
        return f"{statistics.median(ts):.2f} ms ({min(ts):.2f} .. {max(ts):.2f})"

    for case in a.cases.split(","):
        B, L = (int(v) for v in case.split("x"))
        Lp = L // 8
        torch.manual_seed(0)
        net = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=a.layers, dropout=a.dropout, precision="fp32",
                                     trainable=True)
        lit = ClassificationLit(net).to(dev)
        net.dropout_generator = torch.Generator(device=dev).manual_seed(1)
        ids = torch.randint(7, 11, (B, L), device=dev)
        labels = torch.arange(B, device=dev) % 2

        def step(core):
            net.attention_core = core
            lit.zero_grad(set_to_none=True)
            lit.training_step({"input_ids": ids, "labels": labels}).backward()

        lit.train()
        live, failed = {}, {}
        for core in tftrain.CORES:                                    # one step each, alone: peak live bytes, and whether it fits at all
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            try:
                step(core)
                torch.cuda.synchronize()
                live[core] = torch.cuda.max_memory_allocated(dev)
            except torch.cuda.OutOfMemoryError:
                failed[core] = "out of memory"
            lit.zero_grad(set_to_none=True)
        cores = [c for c in tftrain.CORES if c not in failed]
        for _ in range(a.warmup):
            for core in cores:
                step(core)
        ts = {c: [] for c in cores}
        for _ in range(a.steps):                                      # alternating
            for core in cores:
                ts[core].append(event_ms(lambda: step(core)))
        lit.zero_grad(set_to_none=True)
        # one layer's core, on tensors of its shapes
        qkv = torch.randn(B, Lp, 768, device=dev)
        dout = torch.randn(B, Lp, 256, device=dev)
        o, lse = tftrain.attention_forward(qkv, a.dropout, 1)
        t_ef = timed(lambda: tftrain.attention_forward(qkv, a.dropout, 1), a.steps, a.warmup)
        t_eb = timed(lambda: tftrain.attention_backward(qkv, o, lse, dout, a.dropout, 1), a.steps, a.warmup)
        part = f"engine core per layer: forward {fmt(t_ef)}, backward {fmt(t_eb)}, backward / forward {statistics.median(t_eb) / statistics.median(t_ef):.2f}"
        del o, lse
        if "torch" in cores:
            x = qkv.clone().requires_grad_(True)
            t_tf = timed(lambda: tftrain.torch_core(x.detach(), a.dropout), a.steps, a.warmup)
            y = tftrain.torch_core(x, a.dropout)
            t_tb = timed(lambda: torch.autograd.grad(y, x, dout, retain_graph=True), a.steps, a.warmup)
            part += f" | torch core per layer: forward {fmt(t_tf)}, backward {fmt(t_tb)}"
            del x, y
        del qkv, dout
        with torch.no_grad():
            lit.eval()
            t_inf = timed(lambda: lit(ids), a.steps, a.warmup)
        whole = " | ".join([f"whole step, {c} core: {fmt(ts[c])}, live {live[c] / 2 ** 20:.0f} MiB" for c in cores]
                           + [f"whole step, {c} core: {why}" for c, why in failed.items()])
        out(f"transformer {B} x {L} ({Lp} positions, {a.layers} layers, dropout {a.dropout}, {a.steps} steps alternating): {whole} | {part} | "
            f"fp32 inference forward {fmt(t_inf)}")
        net.close()
        del lit, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
