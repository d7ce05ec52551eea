"""Cost of the running verdict (csrc/trajectory.hip): the guarded fp16c step with no request / S = 128 / S = 1024, interleaved in one
process, at the bench shape (256 x 8,193) and the long shape (32 x 32,769).

    python tools/trajectory_bench.py [-o FILE]          # ms per step, median [min .. max] of 5 interleaved samples of 10 steps
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trajectory_bench.py --trace   # S = 128 steps only
"""
import os
import sys
import statistics as st
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from bench import synthetic_ids  # noqa: E402
from chimeralm_amd import lm  # noqa: E402
from chimeralm_amd.engine import TrajectoryRequest  # noqa: E402

TRACE = "--trace" in sys.argv
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.manual_seed(0)
model = lm.ChimeraLM.new(precision="fp16c")
net = model.net
with torch.no_grad():
    for p in net.head.parameters():
        p.mul_(3.0)
eng = net.engine(dev)
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for B, bases, n in ((256, 8192, 10), (32, 32768, 10))[: 1 if TRACE else 2]:      # (the trace: the bench shape alone)
    ids = torch.from_numpy(synthetic_ids(0, B, bases)).to(dev)
    L = bases + 1
    variants = {"none": None, "S=128": TrajectoryRequest(128), "S=1024": TrajectoryRequest(1024)}

    def step(req):
        net.guard(eng, ids)                          # as HyenaDna.forward and bench.py: a self-check where one is due
        eng.forward(ids, trajectory=req)

    for v in variants.values():                      # warm every variant (workspace, code objects)
        step(v)
    torch.cuda.synchronize()
    if TRACE:                                        # the three traj_* kernels run in these steps only: their average per launch
        for _ in range(10):                          # is their cost per step
            step(variants["S=128"])
        torch.cuda.synchronize()
        continue
    ms = {k: [] for k in variants}
    for r in range(5):
        for k, v in variants.items():
            ms[k].append(timed(lambda: step(v), n))
    base = st.median(ms["none"])
    say(f"guarded fp16c {B} x {L}, {n} steps per sample, 5 interleaved samples, ms per step (median [min .. max]):")
    for k in variants:
        say(f"  {k:7s} {st.median(ms[k]):8.3f} [{min(ms[k]):.3f} .. {max(ms[k]):.3f}]   ratio to none {st.median(ms[k]) / base:.4f}")
if "-o" in sys.argv and not TRACE:
    Path(sys.argv[sys.argv.index("-o") + 1]).write_text("\n".join(out) + "\n")
