"""What a training step of the whole HyenaDna net costs on one MI355X, with the Hyena operator's core on the engine and in torch
(chimeralm_amd/hyenatrain.py, csrc/hyena_train.hip, csrc/hyena_longtrain.hip).

    python tools/hyena_train_bench.py [--cases 8x8193,2x32769] [--dropout 0.1] [--warmup 2] [--steps 10] [-o FILE]

The production architecture (lm.ChimeraLM.new), the module's own seeded initialisation, token ids uniform over A/C/G/T.  Timed with
device events on the launch stream.  Where both cores cover the length they run in the same job on the same weights, ALTERNATING step by step (engine, torch, engine, ...), so that clocks and neighbours move both alike; reported per core:
the median of the timed steps and their spread (min .. max).  A step is zero_grad, forward, loss, backward; no optimizer.  Reads of
8,194 to 32,769 tokens alternate the segmented engine op ("engine-long", hyena_long_core="engine") with the torch core in the same
way; longer ones run the torch core alone.  Then, on one layer's tensors: the core forward and backward of the engine
(clm_hyena_train_* or clm_hyena_longtrain_*) and of torch (conv1d, rfft / irfft at n = 2 L, autograd), and the fp32 INFERENCE forward of the
same batch.  Live bytes: torch's peak allocation over one step of each core (the engine's scratch is a torch tensor, so it is
counted).  One line per case, also appended to FILE (profiles/hyena_train_bench.txt is one; profiles/hyena_longtrain_bench.txt is
`--cases 2x32769,4x16385,2x32768`)."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x8193,2x32769")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("-o", "--output")
    a = ap.parse_args()

    def out(line):
        print(line, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(line + "\n")

    import torch

    from chimeralm_amd import hyenatrain as ht, lm

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
        torch.manual_seed(0)
        lit = lm.ChimeraLM.new(precision="fp32", selfcheck=False, trainable=True).to(dev)
        net = lit.net
        net.embed_dropout = a.dropout
        for m in net.head.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = a.dropout
        net.dropout_generator = torch.Generator(device=dev).manual_seed(1)
        torch.manual_seed(1)
        ids = torch.randint(7, 11, (B, L), device=dev)
        labels = torch.arange(B, device=dev) % 2

        def step(core):
            net.hyena_core, net.hyena_long_core = ("engine", "engine") if core == "engine-long" else (core, "torch")
            lit.zero_grad(set_to_none=True)
            lit.training_step({"input_ids": ids, "labels": labels}).backward()

        lit.train()
        wanted = ht.CORES if L <= ht.MAX_ENGINE_TOKENS else ("engine-long", "torch") if L <= ht.MAX_LONG_TOKENS else ("torch",)
        live, failed = {}, {}
        for core in wanted:                                           # one step each, alone: peak live bytes, and whether it fits at all
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            try:
                step(core)
                torch.cuda.synchronize()
                live[core] = torch.cuda.max_memory_allocated(dev)
            except torch.cuda.OutOfMemoryError:
                failed[core] = "out of memory"
            lit.zero_grad(set_to_none=True)
        cores = [c for c in wanted if c not in failed]
        for _ in range(a.warmup):
            for core in cores:
                step(core)
        ts = {c: [] for c in cores}
        for _ in range(a.steps):                                      # alternating
            for core in cores:
                ts[core].append(event_ms(lambda: step(core)))
        lit.zero_grad(set_to_none=True)
        net.hyena_core, net.hyena_long_core = "engine", "torch"
        # one layer's core, on tensors of its shapes and the layer's own filter
        mixer = net.backbone.backbone.layers[0].mixer
        with torch.no_grad():
            k = ht.implicit_filter(mixer, L).contiguous()
            sw, sb, D = mixer.short_filter.weight.squeeze(1).contiguous(), mixer.short_filter.bias.detach(), mixer.filter_fn.bias.detach()
        zc, dy = torch.randn(B, 768, L, device=dev), torch.randn(B, 256, L, device=dev)
        part = ""
        for name, fwd, bwd in (("engine", ht.core_forward, ht.core_backward), ("engine-long", ht.long_core_forward, ht.long_core_backward)):
            if name not in cores:
                continue
            c, _ = fwd(zc, sw, sb, k, D)
            t_ef = timed(lambda: fwd(zc, sw, sb, k, D), a.steps, a.warmup)
            t_eb = timed(lambda: bwd(zc, sw, sb, k, D, c, dy), a.steps, a.warmup)
            part += (f"{name} core per layer: forward {fmt(t_ef)}, backward {fmt(t_eb)}, backward / forward "
                     f"{statistics.median(t_eb) / statistics.median(t_ef):.2f} | ")
            del c
        if "torch" in cores:
            leaves = [t.clone().requires_grad_(True) for t in (zc, sw, sb, k, D)]
            t_tf = timed(lambda: ht.torch_core(zc, sw, sb, k, D), a.steps, a.warmup)
            y = ht.torch_core(*leaves)
            t_tb = timed(lambda: torch.autograd.grad(y, leaves, dy, retain_graph=True), a.steps, a.warmup)
            part += f"torch core per layer: forward {fmt(t_tf)}, backward {fmt(t_tb)} | "
            del leaves, y
        del zc, dy, k
        with torch.no_grad():
            lit.eval()
            t_inf = timed(lambda: lit(ids), a.steps, a.warmup)
        whole = " | ".join([f"whole step, {c} core: {fmt(ts[c])}, live {live[c] / 2 ** 20:.0f} MiB" for c in cores]
                           + [f"whole step, {c} core: {why}" for c, why in failed.items()])
        out(f"hyena {B} x {L} (4 layers, dropout {a.dropout}, {a.steps} steps{' alternating' if len(cores) > 1 else ''}): {whole} | {part}"
            f"fp32 inference forward {fmt(t_inf)}")
        del lit, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
