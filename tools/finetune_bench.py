"""What a step of the head fine-tune costs on one MI355X, part by part: the frozen backbone's forward (which leaves the rows), the
attention pooling forward and backward (csrc/pool_train.hip), the classifier MLP in torch (forward + backward) and the optimizer.

    python tools/finetune_bench.py [--shapes 16x8193,4x32769] [--precisions fp16x3,fp32] [--warmup 3] [--steps 50] [-o FILE]

Seeded weights of the module's own initialisation, token ids uniform over A/C/G/T with [SEP] last.  Each part is timed on its own
with HIP events on the launch stream, median of the timed steps after the warm-up; one line per (precision, shape), also appended to FILE
(profiles/headtrain_bench.txt is one).  The bar the pooling is held to: forward + backward together cost less than the engine
forward of the same micro-batch in the same precision.  FLOPs of the backward on the matrix cores: 2 x 256 x 256 for u and again
for dW1, i.e. 0.26 MFLOP per token, against the fp32 MFMA peak of 157.3 TFLOP/s -- over the time of the whole clm_pool_backward call
(weight pack, tile kernel and reduction of the partials), so the kernel's own share is somewhat higher."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FP32_PEAK = 157.3e12


def timed(fn, warmup, steps, dev):
    st = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x8193,4x32769")
    ap.add_argument("--precisions", default="fp16x3,fp32")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("-o", "--output", default=None)
    a = ap.parse_args()
    from chimeralm_amd import headtrain, lm

    dev = torch.device("cuda", 0)
    lines = []
    for prec in a.precisions.split(","):
        torch.manual_seed(0)
        lit = lm.ChimeraLM.new(precision=prec, selfcheck=False, freeze_backbone=True)
        lit.to(dev)
        net = lit.net.train()
        params = headtrain.head_parameters(lit)
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01)
        att0, att2 = net.head.attention[0], net.head.attention[2]
        for shape in a.shapes.split(","):
            B, L = (int(v) for v in shape.split("x"))
            g = torch.Generator().manual_seed(0)
            ids = torch.randint(7, 11, (B, L), generator=g, dtype=torch.int64)
            ids[:, -1] = 1
            ids = ids.to(dev)
            labels = (torch.arange(B) % 2).to(dev)
            eng = headtrain.train_engine(net, dev)
            t_rows = timed(lambda: eng.forward(ids), a.warmup, a.steps, dev)
            rows = eng.rows()
            w = [att0.weight.detach().contiguous(), att0.bias.detach().contiguous(), att2.weight.detach().view(-1).contiguous(),
                 att2.bias.detach().contiguous()]
            t_fwd = timed(lambda: eng.pool_forward(rows, *w), a.warmup, a.steps, dev)
            scores, stats, pooled = eng.pool_forward(rows, *w)
            dp = torch.randn(B, 256, generator=g).to(dev)
            out = tuple(torch.empty(s, device=dev) for s in ((256, 256), (256,), (256,), (1,)))
            t_bwd = timed(lambda: eng.pool_backward(rows, w[0], w[1], w[2], scores, stats, pooled, dp, out=out), a.warmup, a.steps, dev)

            def mlp():
                x = pooled.detach().requires_grad_(True)
                F.cross_entropy(headtrain.head_mlp(net, x), labels).backward()

            t_mlp = timed(mlp, a.warmup, a.steps, dev)
            for p in params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            t_opt = timed(opt.step, a.warmup, a.steps, dev)

            def step():
                opt.zero_grad(set_to_none=True)
                F.cross_entropy(net(ids), labels).backward()
                opt.step()

            t_step = timed(step, a.warmup, a.steps, dev)
            flop = 2 * 2 * 256 * 256 * B * L
            line = (f"{prec} {B} x {L}: rows forward {t_rows:.3f} ms | pool forward {t_fwd:.3f} ms | pool backward {t_bwd:.3f} ms "
                    f"(call time -- pack, tile kernel and reduce: {flop / (t_bwd / 1e3) / 1e12:.1f} TFLOP/s, {flop / (t_bwd / 1e3) / FP32_PEAK:.2f} of the fp32 MFMA peak) | torch MLP "
                    f"fwd+bwd {t_mlp:.3f} ms | optimizer {t_opt:.3f} ms | whole step {t_step:.3f} ms | pool fwd + bwd = "
                    f"{(t_fwd + t_bwd) / t_rows:.3f} of the rows forward ({'meets' if t_fwd + t_bwd < t_rows else 'MISSES'} the bar)")
            print(line, flush=True)
            lines.append(line)
    if a.output:
        with open(a.output, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
