"""Cost of the test stage against prediction over the same reads, on one MI355X: reads/s of `predict.run_test` (forward + the metric
kernel of csrc/eval_metrics.hip per batch, one read of the sums at the end) and of `predict.run_predict` with a writer that discards
(forward + the logits' copy to the host and a wait for it one batch behind), `model=cnn` at 256 reads x 8,193 synthetic tokens.

    python tools/test_stage_bench.py [--batch 256] [--tokens 8193] [--batches 20] [--rounds 7] [--warmup 1]

The CNN's forward is the shortest of the nets, so a wait per batch would show most here.  Both loops run in one process, interleaved
round by round (predict, test, predict, test, ...), each round timed on the host clock from before its first batch to after its last
wait, device idle before and after; median and minimum over the rounds are reported as one JSON line.  Both loops pay the same host
work per batch (ids to bytes, page-locked staging, the H2D copy); the same collated batch object is served every time, so the
loader itself costs nothing."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


class _Loader:
    def __init__(self, batch: dict, n: int, rows: int):
        self.batch, self.n, self.batch_size_per_device = batch, n, rows

    def _it(self):
        return (self.batch for _ in range(self.n))

    test_dataloader = predict_dataloader = _it


class _Discard:
    def write_on_batch_end(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=8193)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.cnn import DNAConvNet
    from chimeralm_amd.eval_metrics import EvalMetrics
    from chimeralm_amd.predict import run_predict, run_test

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                     hidden_dim=512, number_of_classes=2)
    model = ClassificationLit(net)
    batch = {"input_ids": torch.randint(7, 11, (a.batch, a.tokens), generator=g, dtype=torch.int64),
             "labels": torch.randint(0, 2, (a.batch,), generator=g, dtype=torch.int64)}
    loader = _Loader(batch, a.batches, a.batch)
    metrics = EvalMetrics(dev, ignore_index=model.test_criterion())
    model.test_metrics = metrics
    reads = a.batch * a.batches

    def predict_round():
        return run_predict(model, loader, _Discard(), dev)

    def test_round():
        metrics.reset()
        n = run_test(model, loader, dev)
        r = metrics.read()
        assert r["n_valid"] == n and r["n_batches"] == a.batches
        return n

    rate = {"predict": [], "test": []}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in (("predict", predict_round), ("test", test_round)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            assert n == reads
            if rnd >= a.warmup:
                rate[name].append(reads / dt)
    out = {"net": "DNAConvNet", "batch": a.batch, "tokens": a.tokens, "batches_per_round": a.batches, "rounds": a.rounds}
    for name, v in rate.items():
        out[name] = {"median_reads_per_s": round(statistics.median(v), 1), "min_reads_per_s": round(min(v), 1),
                     "max_reads_per_s": round(max(v), 1), "rounds": [round(x, 1) for x in v]}
    out["test_over_predict_median"] = round(out["test"]["median_reads_per_s"] / out["predict"]["median_reads_per_s"], 4)
    print(json.dumps(out), flush=True)
    metrics.close()
    net.close()


if __name__ == "__main__":
    main()
