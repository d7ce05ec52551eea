"""End-to-end `predict` throughput on a synthetic BAM: native feeder -> staged H2D -> engine -> prediction files, one GPU.

    python tools/e2e_bench.py [--reads 6000] [--bases 8192] [--batch 256] [--precision fp16c]
    python tools/e2e_bench.py --bam tests/golden/test_chimric_reads.bam --batch 12 --repeat 5     (a real, ragged file: the reference's)
    python tools/e2e_bench.py ... --long-reads tile      (reads beyond the context in overlapping windows: predict --long-reads tile)
    python tools/e2e_bench.py ... --batching bucket      (reads regrouped by canonical length: predict --batching bucket)
    python tools/e2e_bench.py --ragged --reads 3000      (synthetic file, seeded log-uniform lengths of 500 ... 32,768 bases)

Same loop as `python -m chimeralm_amd predict` (chimeralm_amd.predict.run_predict_native) with seeded random weights; the
clock starts after the first batch (filters / workspace for the length are built on it) and stops when the last prediction
file is written."""
from __future__ import annotations

import argparse
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=6000)
    ap.add_argument("--bases", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", default="fp16c")
    ap.add_argument("--min-bases", type=int, default=None, help="ragged file: read lengths uniform in [min-bases, bases]")
    ap.add_argument("--bam", type=Path, default=None, help="a real BAM instead of the synthetic one (batches padded on the left to their longest read)")
    ap.add_argument("--repeat", type=int, default=3, help="--bam: timed passes over the file after one warm-up pass")
    ap.add_argument("--long-reads", choices=("truncate", "tile"), default="truncate", help="as predict --long-reads (tile: the defaults)")
    ap.add_argument("--batching", choices=("file", "bucket"), default="file", help="as predict --batching (bucket: the defaults)")
    ap.add_argument("--ragged", action="store_true", help="synthetic file: seeded log-uniform read lengths of 500 ... 32,768 bases")
    ap.add_argument("--net", choices=("hyena", "mambasp"), default="hyena", help="the net: the Hyena model (--precision applies) or "
                    "configs/model/mambasp.yaml's (synthetic files only, through the Python data path), both with seeded random weights")
    a = ap.parse_args()
    from feeder_bench import write_bam

    from chimeralm_amd import lm
    from chimeralm_amd.callbacks import PredictionWriter
    from chimeralm_amd.feeder import BamFeeder
    from chimeralm_amd.longread import Options
    from chimeralm_amd.predict import run_predict_native

    tile = Options() if a.long_reads == "tile" else None
    bucket = None
    if a.batching == "bucket":
        from chimeralm_amd.bucket import Options as BucketOptions

        import logging

        bucket = BucketOptions()
        logging.basicConfig(level=logging.INFO, format="%(message)s")      # the loop's line with the tokens it forwarded
    tag = (lambda label: label) if tile is None else (lambda label: f"{label} (long reads tiled)")
    if bucket is not None:
        tag = lambda label: f"{label} (bucketed)"                          # noqa: E731
    feed = {} if tile is None else {"max_tokens": tile.max_tokens}         # untruncated rows: the windows are cut on the device
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    if a.net == "hyena":
        model = lm.ChimeraLM.new(precision=a.precision)
    else:
        from chimeralm_amd.basic_module import ClassificationLit
        from chimeralm_amd.mamba import MambaSequenceClassificationSP

        model = ClassificationLit(MambaSequenceClassificationSP(vocab_size=12, embedding_dim=512, number_of_layers=3, dropout=0.2, headdim=64,
                                                                d_state=128, d_conv=4, expand=3, number_of_classes=2, precision="fp16x3"))
    if a.bam is not None:
        # one warm-up pass (filters, workspace, the guard's first hearing, the [PAD] tables), then `repeat` timed passes; with the
        # share of tail tiles that lie wholly inside a [PAD] prefix (what csrc/pad_prefix.hip does not compute)
        import os

        import numpy as np

        with tempfile.TemporaryDirectory() as td:
            tiles = pad_tiles = toks = pads = 0
            with BamFeeder(a.bam, batch_size=a.batch) as f:
                while True:
                    fb = f.next()
                    if fb is None:
                        break
                    ids = np.asarray(fb.ids[:, : fb.n_tokens])
                    lead = (ids == 4).cumprod(axis=1).sum(axis=1)
                    tiles += ids.shape[0] * ((ids.shape[1] + 127) // 128)
                    pad_tiles += int((lead // 128).sum())
                    toks += ids.size
                    pads += int(lead.sum())
                    f.release(fb)
            print(f"{a.bam.name} at batch {a.batch}: {toks:,} tokens, {pads / toks:.1%} of them leading [PAD]; {tiles:,} tail tiles, "
                  f"{pad_tiles / tiles:.1%} wholly inside a [PAD] prefix; CLM_DEBUG={os.environ.get('CLM_DEBUG', '')!r}")
            for label, reps in (("warm-up", 1), ("timed", a.repeat)):
                t0, done = time.perf_counter(), 0
                for r in range(reps):
                    with BamFeeder(a.bam, batch_size=a.batch, **feed) as f:
                        done += run_predict_native(model, f, PredictionWriter(Path(td) / f"pred_{label}_{r}"), device, long_reads=tile,
                                                   batching=bucket)
                dt = time.perf_counter() - t0
                print(f"{tag(label)}: {done} reads in {reps} pass(es), {dt:.2f} s -> {done / dt:,.0f} reads/s end to end")
            print("guard:", {k: v for k, v in (getattr(model.net, "selfcheck_report", None) or {}).items() if k != "samples"})
        return
    with tempfile.TemporaryDirectory() as td:
        path = Path(td) / "synthetic.bam"
        lengths = None
        if a.ragged:
            import numpy as np

            lengths = np.exp(np.random.default_rng(1).uniform(np.log(500), np.log(32768), a.reads)).round().astype(np.int64)
            file_tokens = sum(min(a.batch, a.reads - i) * (int(lengths[i: i + a.batch].max()) + 1) for i in range(0, a.reads, a.batch))
            print(f"ragged file: {a.reads} reads, {int(lengths.sum()) + a.reads:,} tokens, {lengths.min():,} ... {lengths.max():,} bases; "
                  f"batches of {a.batch} in file order hold {file_tokens:,} tokens")
        write_bam(path, a.reads, a.bases, min_bases=a.min_bases, lengths=lengths)
        for label, n in (("warm-up", 2 * a.batch), ("timed", None)):
            out = Path(td) / f"pred_{label}"
            t0 = time.perf_counter()
            if a.net != "hyena":                   # the native loop drives the Hyena engine's own staging: other nets take the Python data path
                from chimeralm_amd import bam, tokenizer
                from chimeralm_amd.predict import run_predict

                dm = bam.BamDataModule(tokenizer=tokenizer.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen"),
                                       predict_data_path=path, batch_size=a.batch, max_predict_samples=n)
                dm.setup("predict")
                done = run_predict(model, dm, PredictionWriter(out), device, batching=bucket)
            else:
                with BamFeeder(path, batch_size=a.batch, max_reads=n, **feed) as f:
                    done = run_predict_native(model, f, PredictionWriter(out), device, long_reads=tile, batching=bucket)
            dt = time.perf_counter() - t0
            files = len(list(out.glob("*.txt")))
            print(f"{tag(label)}: {done} reads, {files} prediction files, {dt:.2f} s -> {done / dt:,.0f} reads/s end to end")
            if label == "timed" and getattr(model.net, "selfcheck_report", None):
                print("guard:", {k: v for k, v in model.net.selfcheck_report.items() if k != "samples"})


if __name__ == "__main__":
    main()
