"""What a training step of the two Mamba nets costs on one MI355X, part by part (chimeralm_amd/mambatrain.py, csrc/mamba_train.hip).

    python tools/mamba_train_bench.py [--cases mamba:8x8193,mambasp:8x8193,mambasp:4x32769] [--warmup 3] [--steps 50] [-o FILE]
    rocprofv3 --output-format csv --kernel-trace --stats -d DIR -- python tools/mamba_train_bench.py --cases mambasp:8x8193 --steps 5 --no-alt
                                                                                                             (a run of its own)
    python tools/mamba_train_bench.py --kernel-stats DIR/.../*_kernel_stats.csv [-o FILE]                    (no GPU needed)

The nets in their config sizes (configs/model/mamba.yaml, mambasp.yaml), the module's own seeded initialisation, token ids uniform
over A/C/G/T, dropout as configured.  The first form times with device events on the launch stream (median of the timed steps after
the warm-up): the whole step (zero_grad, forward, loss, backward; no optimizer), and on ONE layer's tensors the core forward
(clm_mamba_train_forward), the core backward (clm_mamba_train_backward) and the torch projections (in_proj + out_proj, forward and
backward).  In the same call it measures the two yardsticks: the exact-fp32 INFERENCE forward of the same batch, and the only
alternative a user has without this op -- torch autograd through the chunked scan written in torch ops (tests/mamba_reference.py
`scan_chunked`, via tests/mamba_train_reference.py `core_forward`) on the GPU in fp32 with the same projections, one step.  Live
bytes: torch's peak allocation over a step plus the engine's scratch.  One line per case, also appended to FILE
(profiles/mamba_train_bench.txt is one).

Kernel times come from rocprofv3 in a run of its own (tracing slows the host); the third form reads its kernel statistics and prints
calls, mean and total of every mtrain_* kernel and the share of each in their sum."""
from __future__ import annotations

import argparse
import csv
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

NETS = {
    "mamba": dict(embedding_dim=256, number_of_layers=12, model_max_length=30000, dropout=0.1, d_state=16, expand=2),
    "mambasp": dict(embedding_dim=512, number_of_layers=3, dropout=0.2, d_state=128, expand=3),
}


def kernel_stats(path: str, out):
    rows = list(csv.DictReader(open(path)))
    name_col = next(c for c in rows[0] if c.lower() in ("name", "kernelname", "kernel_name"))
    calls_col = next(c for c in rows[0] if c.lower() == "calls")
    total_col = next(c for c in rows[0] if c.lower().startswith("totalduration"))
    mine = [(r[name_col].split("mtrain_", 1)[1].split("(")[0], int(r[calls_col]), float(r[total_col]) / 1e6) for r in rows if "mtrain_" in r[name_col]]
    whole = sum(t for _, _, t in mine)
    out("\n".join(f"mtrain_{n}: {c} launches, mean {t / c * 1e3:.1f} us, total {t:.3f} ms, {t / whole:.1%} of the mtrain_* kernels"
                  for n, c, t in sorted(mine, key=lambda x: -x[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="mamba:8x8193,mambasp:8x8193,mambasp:4x32769")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-alt", action="store_true", help="skip the torch-autograd alternative (profiling runs)")
    ap.add_argument("--kernel-stats")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()

    def out(line):
        print(line, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(line + "\n")

    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, out)

    import torch
    import torch.nn.functional as F

    from chimeralm_amd import mambatrain
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.mamba import MambaSequenceClassification, MambaSequenceClassificationSP

    dev = torch.device("cuda", 0)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    for case in a.cases.split(","):
        name, shape = case.split(":")
        B, L = (int(v) for v in shape.split("x"))
        kw = NETS[name]
        torch.manual_seed(0)
        cls = MambaSequenceClassification if name == "mamba" else MambaSequenceClassificationSP
        net = cls(vocab_size=12, number_of_classes=2, precision="fp32", trainable=True, **kw)
        lit = ClassificationLit(net).to(dev)
        ids = torch.randint(7, 11, (B, L), device=dev)
        labels = torch.arange(B, device=dev) % 2
        d, nl, N, ex = kw["embedding_dim"], kw["number_of_layers"], kw["d_state"], kw["expand"]

        def step():
            lit.zero_grad(set_to_none=True)
            lit.training_step({"input_ids": ids, "labels": labels}).backward()

        lit.train()
        torch.cuda.reset_peak_memory_stats(dev)
        t_step = timed(step, a.steps, a.warmup)
        live = torch.cuda.max_memory_allocated(dev) + mambatrain.workspace_bytes(B, L, d, ex, N)
        lit.zero_grad(set_to_none=True)
        # one layer's parts, on tensors of its shapes
        layer = net._layer(0)
        eng = net.train_engine(dev)
        params = [p.detach() for p in mambatrain.core_parameters(layer)]
        h = torch.randn(B, L, d, device=dev)
        zx = F.linear(h, layer.in_proj.weight).detach()
        out_, saved = eng.forward(zx, params, d, ex, N)
        dout = torch.randn_like(out_)
        t_cf = timed(lambda: eng.forward(zx, params, d, ex, N), a.steps, a.warmup)
        t_cb = timed(lambda: eng.backward(zx, params, saved, dout, d, ex, N), a.steps, a.warmup)

        def proj():
            hh = h.detach().requires_grad_(True)
            z = F.linear(hh, layer.in_proj.weight)
            y = F.linear(out_.detach().requires_grad_(True), layer.out_proj.weight)
            torch.autograd.backward([z, y], [torch.ones_like(z), torch.ones_like(y)])
            layer.zero_grad(set_to_none=True)

        t_proj = timed(proj, a.steps, a.warmup)
        del out_, saved, dout, zx, h
        with torch.no_grad():
            lit.eval()
            t_inf = timed(lambda: lit(ids), a.steps, a.warmup)
        line = (f"{name} {B} x {L} (d {d}, {nl} layers, N {N}, expand {ex}): whole step {t_step:.2f} ms ({B / t_step * 1e3:.1f} reads/s) | per layer: "
                f"core forward {t_cf:.3f} ms, core backward {t_cb:.3f} ms ({t_cb / t_cf:.2f} x its forward), torch projections fwd+bwd "
                f"{t_proj:.3f} ms | x {nl} layers: core {nl * (t_cf + t_cb):.2f} ms, projections {nl * t_proj:.2f} ms, the rest "
                f"{t_step - nl * (t_cf + t_cb + t_proj):.2f} ms | fp32 inference forward {t_inf:.2f} ms: step = {t_step / t_inf:.2f} x | "
                f"live {live / 2 ** 20:.0f} MiB")
        if not a.no_alt:
            import mamba_train_reference as R

            def alt():
                lit.zero_grad(set_to_none=True)
                x = net.embedding(ids)
                if hasattr(net, "input_block"):
                    x = net.input_block(x + net.pos_embedding[:, :L])
                for i in range(nl):
                    ly = net._layer(i)
                    p = dict(zip(R.CORE_PARAMS, mambatrain.core_parameters(ly)))
                    x = x + F.linear(R.core_forward(F.linear(x, ly.in_proj.weight), p), ly.out_proj.weight)
                pooled = (x.mean(1) + x.max(1)[0]) / 2
                F.cross_entropy(net.classifier(net.pooler(pooled)), labels).backward()

            lit.train()
            try:
                torch.cuda.reset_peak_memory_stats(dev)
                t_alt = timed(alt, max(1, min(a.steps, 3)), 1)
                line += (f" | torch autograd through scan_chunked (fp32, same projections): {t_alt:.1f} ms, {t_alt / t_step:.1f} x the step, "
                         f"live {torch.cuda.max_memory_allocated(dev) / 2 ** 20:.0f} MiB")
            except torch.cuda.OutOfMemoryError:
                line += " | torch autograd through scan_chunked: out of memory"
        out(line)
        lit.zero_grad(set_to_none=True)
        net.close()
        del lit, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
