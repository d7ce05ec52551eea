"""`chimeralm predict` for the MI355X engine -- same options as /root/reference/chimeralm/__main__.py:248-259:

    python -m chimeralm_amd predict DATA_PATH [-g GPUS] [-o OUTPUT] [-b BATCH] [-w WORKERS] [-c CKPT] [-r] [-v]
                                              [--long-reads truncate|tile --long-overlap 4096 --long-max-bases 262144]
                                              [--batching file|bucket --bucket-steps 3]
                                              [--save-trajectory --trajectory-stride 128 --trajectory-values]

plus engine-only options `--weights` (directory/file with the released `model.safetensors`; the reference downloads
`yangliz5/chimeralm` from the Hub) and `--precision`.  `--gpus 0` (the reference's CPU mode) is refused: this engine
has no CPU path.  `filter` (reference :320-331) is the host-only step after predict; `web` is not built.

    python -m chimeralm_amd explain DATA_PATH [-o OUTPUT] [--max-reads N] [--window W --stride S --substitute N|all --score prob|gap
                                              --top-k K --values] [--weights DIR | --ckpt FILE] [--precision P]

has no command in the reference: it is `Mamba2Analyzer.get_position_importance` (chimeralm/explain/motif.py:64-82) as an engine
capability, for the released Hyena model (`python explain.py model=...` at the repository's root serves every net).

    python -m chimeralm_amd finetune TRAIN.parquet [--val VAL.parquet] [-o OUT] [--epochs 10 --lr 1e-4 -b 16 --precision fp16x3
                                              --seed 12345] [--weights DIR | --ckpt FILE]

is the reference's `train.py` with `freeze_backbone=True`, cut down to one GPU: the classifier head is fitted to labelled reads, the
backbone stays as released (headtrain.py).

    python -m chimeralm_amd train TRAIN.parquet [--val VAL.parquet] [-o OUT] [--epochs 10 --lr 1e-4 -b 8 --seed 12345] [--ckpt FILE]

is the reference's `train.py` with its default `model=cnn`, cut down to one GPU: DNAConvNet is trained end to end, forward and
backward on the engine (cnntrain.py); `python eval.py ckpt_path=OUT/model.safetensors model=cnn ...` then runs the result.
`--net mamba` / `--net mambasp` trains the reference's Mamba nets instead (mambatrain.py: the Mamba2 core forward and backward on the
engine, the projections in torch); `python eval.py ckpt_path=OUT/model.safetensors model=mambasp ...` runs that result.
"""
from __future__ import annotations

import logging
import os
import subprocess
import sys
from pathlib import Path

import torch
import typer

app = typer.Typer(context_settings={"help_option_names": ["-h", "--help"]},
                  help="ChimeraLM predict on AMD MI355X: flag chimera artifacts from whole genome amplification.")
log = logging.getLogger("chimeralm_amd")


@app.callback()
def main():
    """ChimeraLM (MI355X engine)."""


@app.command()
def predict(
    data_path: Path = typer.Argument(..., help="Path to the dataset (BAM)"),
    gpus: int = typer.Option(1, "--gpus", "-g", help="Number of GPUs to use"),
    output_path: Path | None = typer.Option(None, "--output", "-o", help="Output path for predictions"),
    batch_size: int = typer.Option(12, "--batch-size", "-b", help="Batch size"),
    num_workers: int = typer.Option(0, "--workers", "-w", help="Number of workers"),
    ckpt_path: Path | None = typer.Option(None, "--ckpt", "-c", hidden=True, help="Path to the checkpoint file"),
    weights: str = typer.Option("yangliz5/chimeralm", "--weights", help="Directory/file with model.safetensors"),
    precision: str = typer.Option("fp16c", "--precision", help="arithmetic of the dense projections: fp16c (default: fp16 activations x fp16 hi + fp8 lo weights -- MLP weights plain fp16 -- at 16-bit MFMA rate, checked against the exact-fp32 kernels on the loaded weights before the first batch, replaced by them if more than --selfcheck-tol off) | fp32 (exact, the reference's) | fp16x3 (every operand as two halfs, three fp16 MFMAs per product: fp32-class accuracy at twice the exact rate, no check needed) | fp16 | bf16 (reduced precision)"),
    selfcheck_tol: float = typer.Option(5e-4, "--selfcheck-tol", help="largest |logit difference| from exact fp32 the fp16c mode may show in its self-check (0 disables the check)"),
    feeder: str = typer.Option("native", "--feeder", help="BAM input: native (C++ decoder thread, pinned ring) | python"),
    random: bool = typer.Option(False, "--random", "-r", help="Make the prediction not deterministic"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose output"),
    gather_logits: bool = typer.Option(False, "--gather-logits", help="multi-GPU: all-gather every batch's logits (RCCL, side "
                                       "stream) and let rank 0 also write them to logits.tsv (batch, rank, row, logit0, logit1)"),
    save_attention: bool = typer.Option(False, "--save-attention", help="also write {rank}_{batch}.attn.tsv per batch: per read its "
                                        "label, number of bases and pads, the pooling weight on pads and on [SEP], and the bases "
                                        "of largest pooling weight as pos:weight (where in the read the model looked)"),
    attention_top_k: int = typer.Option(10, "--attention-top-k", help="bases listed per read by --save-attention (1 ... 32)"),
    attention_weights: bool = typer.Option(False, "--attention-weights", help="with --save-attention (implied): also write "
                                           "{rank}_{batch}.attn.npz with the pooling weight of every base of every read"),
    save_trajectory: bool = typer.Option(False, "--save-trajectory", help="also write {rank}_{batch}.traj.tsv per batch: the verdict as "
                                         "a function of how much of the read has been seen -- per read the bases seen where its label "
                                         "settles and either side of the largest step towards it -- from the one forward predict runs "
                                         "anyway.  Whether these points track a real junction has not been measured"),
    trajectory_stride: int = typer.Option(128, "--trajectory-stride", help="--save-trajectory: tokens between two points (a multiple of "
                                          "128 in 128 ... 4096)"),
    trajectory_values: bool = typer.Option(False, "--trajectory-values", help="with --save-trajectory (implied): also write "
                                           "{rank}_{batch}.traj.npz with the logits at every point of every read"),
    long_reads: str = typer.Option("truncate", "--long-reads", help="reads longer than the model's context (32,768 bases): truncate "
                                   "(the reference's: only the first 32,768 bases are seen) | tile: cut them into overlapping "
                                   "context-sized windows, judge every window, call the read an artifact if any window is one and "
                                   "write {rank}_{batch}.windows.tsv with every window's logits.  How well the model judges a window "
                                   "cut from the middle of a read has not been measured: it was trained on read starts"),
    long_overlap: int = typer.Option(4096, "--long-overlap", help="--long-reads tile: bases two consecutive windows share (0 ... half "
                                     "the window; a choice, not a tuned value)"),
    long_max_bases: int = typer.Option(262144, "--long-max-bases", help="--long-reads tile: bases of a read that are looked at; the "
                                       "rest is cut off and counted by the feeder (truncated_bases)"),
    long_window: int | None = typer.Option(None, "--long-window", hidden=True, help="--long-reads tile: bases per window (default: "
                                           "the tokenizer's length; for tests and checkpoints of a shorter context)"),
    batching: str = typer.Option("file", "--batching", help="how batches are formed: file (the reference's: reads in file order, "
                                 "every batch padded to its longest read, so a read's logits depend on its batch-mates) | bucket: "
                                 "every read is padded to a canonical length of its own and reads of one such length are forwarded "
                                 "together -- the verdict on a read does not depend on -b, -g or the reads around it, and a ragged "
                                 "file pays for few pads.  The pads differ from the reference's: not reference parity.  File "
                                 "{rank}_{k}.txt is then the rank's k-th emitted batch"),
    bucket_steps: int = typer.Option(3, "--bucket-steps", help="--batching bucket: log2 of the canonical lengths per octave above "
                                     "1,024 bases (0 ... 5; 3: at most an eighth of a row is pads)"),
):
    """Predict the given dataset using ChimeraLM."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s")
    if gpus < 1:
        raise typer.BadParameter("this engine runs on MI355X GPUs only; use --gpus >= 1 (no CPU path exists)")
    if batching not in ("file", "bucket"):
        raise typer.BadParameter("--batching must be file or bucket")
    bucket = None
    if batching == "bucket":
        if long_reads == "tile":
            raise typer.BadParameter("--batching bucket and --long-reads tile exclude each other: a window plan is made per "
                                     "file-order batch")
        if gather_logits:
            raise typer.BadParameter("--batching bucket and --gather-logits exclude each other: logits.tsv identifies a read by its "
                                     "position in a file-order batch, which a regrouped batch does not have")
        from .bucket import Options as BucketOptions

        try:
            bucket = BucketOptions(mode="bucket", steps_log2=bucket_steps)
        except ValueError as e:
            raise typer.BadParameter(f"--bucket-steps: {e}") from None
    save_attention = save_attention or attention_weights
    if save_attention and not 1 <= attention_top_k <= 32:
        raise typer.BadParameter("--attention-top-k must be 1 ... 32")
    if long_reads not in ("truncate", "tile"):
        raise typer.BadParameter("--long-reads must be truncate or tile")
    save_trajectory = save_trajectory or trajectory_values
    if save_trajectory:
        if long_reads == "tile":
            raise typer.BadParameter("--long-reads tile and --save-trajectory exclude each other: a read reduced from several windows "
                                     "has no single row to follow")
        from .engine import check_trajectory_stride

        try:
            check_trajectory_stride(trajectory_stride)
        except ValueError as e:
            raise typer.BadParameter(f"--trajectory-stride: {e}") from None
    tile = None
    if long_reads == "tile":
        if save_attention:
            raise typer.BadParameter("--long-reads tile and --save-attention exclude each other: the pooling weights of a read "
                                     "reduced from several windows are not defined")
        from .longread import Options as LongReadOptions

        try:
            tile = LongReadOptions(mode="tile", window=long_window, overlap=long_overlap, max_bases=long_max_bases)
        except ValueError as e:
            raise typer.BadParameter(f"--long-reads tile: {e}") from None
    if output_path is None:                       # README-documented default (the reference crashes here)
        output_path = data_path.with_suffix(".predictions")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if gpus > 1 and world == 1:                   # one process per GPU, launched before anything touches HIP
        from .distributed import free_port

        port = os.environ.get("MASTER_PORT") or str(free_port())      # a port that is free now, not a fixed one
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
               "--master-addr", "127.0.0.1", "--master-port", port, "-m", "chimeralm_amd", *sys.argv[1:]]
        raise typer.Exit(subprocess.call(cmd))

    from . import bam, callbacks, distributed, lm, predict as loop, tokenizer

    # CLM_DIST_BACKEND=gloo with CLM_RANKS_SHARE_GPU=1 is the one-GPU rehearsal of a multi-GPU run (tests/test_gpu_multirank.py):
    # RCCL refuses two ranks per device, everything else is the real path
    backend = os.environ.get("CLM_DIST_BACKEND")
    rank, local_rank, world = distributed.init_process_group(backend)
    if not random:
        torch.manual_seed(42)
    device = torch.device("cuda", local_rank % torch.cuda.device_count() if os.environ.get("CLM_RANKS_SHARE_GPU") == "1" else local_rank)
    torch.cuda.set_device(device)
    tok = tokenizer.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    if feeder not in ("native", "python"):
        raise typer.BadParameter("--feeder must be native or python")
    if batch_size % world != 0:                   # bam.py:142-146
        raise RuntimeError(f"Batch size ({batch_size}) is not divisible by the number of devices ({world}).")
    if ckpt_path is not None:
        log.info(f"Loading model from {ckpt_path}")
        model = lm.ChimeraLM.new(precision=precision, selfcheck=None if selfcheck_tol > 0 else False, selfcheck_tol=selfcheck_tol,
                                 attention_top_k=attention_top_k if save_attention else None,
                                 trajectory_stride=trajectory_stride if save_trajectory else None).load_reference_checkpoint(ckpt_path)
    else:
        log.info(f"Loading model weights {weights}")
        model = lm.ChimeraLM.from_pretrained(weights, precision=precision, selfcheck=None if selfcheck_tol > 0 else False,
                                             selfcheck_tol=selfcheck_tol, attention_top_k=attention_top_k if save_attention else None,
                                             trajectory_stride=trajectory_stride if save_trajectory else None)
    output_path.mkdir(parents=True, exist_ok=True)
    writer = callbacks.PredictionWriter(output_dir=output_path, write_interval="batch")
    attn_writer = callbacks.AttentionWriter(output_dir=output_path, weights=attention_weights) if save_attention else None
    traj_writer = callbacks.TrajectoryWriter(output_dir=output_path, values=trajectory_values) if save_trajectory else None
    if feeder == "native":
        from .feeder import BamFeeder

        max_tokens, slots = tok.max_len_single_sentence if tile is None else tile.max_tokens, 4
        if bucket is not None and tok.padding_side != "left":
            raise typer.BadParameter("--batching bucket takes batches padded on the left only")
        if tile is not None:
            if tok.padding_side != "left":
                raise typer.BadParameter("--long-reads tile takes batches padded on the left only")
            log.info(f"[rank {rank}] long reads: windows of {tile.window_bases:,} bases, overlap {tile.overlap:,}, up to {tile.max_bases:,} "
                     f"bases per read; feeder ring {slots} x {batch_size // world} x {max_tokens:,} = "
                     f"{slots * (batch_size // world) * max_tokens / 1e6:,.0f} MB page-locked")
        with BamFeeder(data_path, batch_size=batch_size // world, max_tokens=max_tokens, slots=slots, rank=rank,
                       world=world, pad_left=tok.padding_side == "left") as fd:
            n = loop.run_predict_native(model, fd, writer, device, rank=rank, gather=world > 1 and gather_logits,
                                        on_batch=_gathered_sink(output_path, rank) if gather_logits else None,
                                        attention_writer=attn_writer, long_reads=tile, batching=bucket, trajectory_writer=traj_writer)
            log.info(f"[rank {rank}] feeder: {fd.stats()}")
    else:
        dm = bam.BamDataModule(tokenizer=tok, train_data_path=Path("dummy.bam"), predict_data_path=data_path,
                               batch_size=batch_size, num_workers=num_workers, max_length=None if tile is None else tile.max_tokens)
        dm.setup("predict", world_size=world, rank=rank)
        n = loop.run_predict(model, dm, writer, device, rank=rank, gather=world > 1 and gather_logits,
                             on_batch=_gathered_sink(output_path, rank) if gather_logits else None, attention_writer=attn_writer,
                             long_reads=tile, batching=bucket, trajectory_writer=traj_writer)
    distributed.barrier()
    rep = getattr(model.net, "selfcheck_report", None)
    if rep:
        log.info(f"[rank {rank}] precision {precision}: self-check against exact fp32 max |dlogit| {rep.get('max_abs_dlogit', 0.0):.2e} "
                 f"(threshold {rep.get('tol')}) -> {('FELL BACK to ' + rep.get('fallback_precision', 'fp16x3')) if rep.get('fallback') else 'kept'}")
    log.info(f"[rank {rank}] {n} reads; predictions saved to {output_path}")


def _gathered_sink(output_path: Path, rank: int):
    """Rank 0 appends the gathered [B, 2] logits of every batch to <output>/logits.tsv; rows are in rank order (rank r's
    shard of batch b are rows r*B/G .. (r+1)*B/G - 1)."""
    if rank != 0:
        return lambda batch_idx, gathered: None
    f = (output_path / "logits.tsv").open("w")

    def sink(batch_idx: int, gathered):
        rows = gathered.shape[0] // max(1, int(os.environ.get("WORLD_SIZE", "1")))
        for i, row in enumerate(gathered.tolist()):
            if row[2] > 0:                                    # rows of short / empty batches are padding
                f.write(f"{batch_idx}\t{i // rows}\t{i % rows}\t{row[0]:.7g}\t{row[1]:.7g}\n")
        f.flush()
    return sink


@app.command()
def explain(
    data_path: Path = typer.Argument(..., help="Path to the dataset (BAM)"),
    output_path: Path | None = typer.Option(None, "--output", "-o", help="Output directory (default: DATA_PATH with suffix .explain)"),
    max_reads: int | None = typer.Option(None, "--max-reads", help="scan only the first N reads"),
    window: int = typer.Option(1, "--window", help="bases replaced together (>= 1)"),
    stride: int = typer.Option(1, "--stride", help="distance between window starts (1 ... window)"),
    substitute: str = typer.Option("N", "--substitute", help="N: the window's bases become N | all: saturation mutagenesis, every "
                                   "base becomes each of the other three (needs --window 1 --stride 1)"),
    score: str = typer.Option("prob", "--score", help="prob: |change of p1| (the reference's number; vanishes on confident reads) | "
                              "gap: |change of logit1 - logit0|"),
    top_k: int = typer.Option(10, "--top-k", help="bases listed per read (1 ... 32)"),
    values: bool = typer.Option(False, "--values", help="also write {rank}_{index}.explain.npz per read with logits, dp1, dgap, "
                                "importance and peaks"),
    batch_size: int = typer.Option(256, "--batch-size", "-b", help="mutants per forward"),
    ckpt_path: Path | None = typer.Option(None, "--ckpt", "-c", help="Path to the checkpoint file"),
    weights: str = typer.Option("yangliz5/chimeralm", "--weights", help="Directory/file with model.safetensors"),
    precision: str = typer.Option("fp16x3", "--precision", help="arithmetic of the dense projections: fp16x3 (default) | fp32 | fp16c | "
                                  "fp16 | bf16.  The default is NOT predict's fp16c: fp16c may be up to 5e-4 off in a logit, and a "
                                  "scan reports DIFFERENCES of logits between a read and its mutants -- that error is a noise floor "
                                  "under the signal; fp16x3 stays within ~1e-5"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose output"),
):
    """In-silico mutagenesis: which bases of each read the prediction rests on (writes {rank}_explain.tsv)."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s")
    from . import explain as ex

    try:
        opts = ex.Options(window=window, stride=stride, substitute=substitute, score=score, top_k=top_k)
    except ValueError as e:
        raise typer.BadParameter(str(e)) from None
    if max_reads is not None and max_reads < 1:
        raise typer.BadParameter("--max-reads must be >= 1")
    if not 1 <= batch_size <= 65535:
        raise typer.BadParameter("--batch-size must be 1 ... 65535")
    if output_path is None:
        output_path = data_path.with_suffix(".explain")

    from . import bam, callbacks, lm, predict as loop, tokenizer

    torch.manual_seed(42)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    tok = tokenizer.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    kw = dict(precision=precision, selfcheck=None)
    if ckpt_path is not None:
        log.info(f"Loading model from {ckpt_path}")
        model = lm.ChimeraLM.new(**kw).load_reference_checkpoint(ckpt_path)
    else:
        log.info(f"Loading model weights {weights}")
        model = lm.ChimeraLM.from_pretrained(weights, **kw)
    dm = bam.BamDataModule(tokenizer=tok, train_data_path=Path("dummy.bam"), predict_data_path=data_path, batch_size=12, num_workers=0,
                           max_predict_samples=max_reads)
    dm.setup("predict", world_size=1, rank=0)
    writer = callbacks.ExplainWriter(output_dir=output_path, values=values)
    n = loop.run_explain(model, dm, writer, device, max_reads=max_reads, batch_size=batch_size, window=opts.window, stride=opts.stride,
                         substitute=opts.substitute, score=opts.score, top_k=opts.top_k)
    log.info(f"{n} reads scanned; results saved to {output_path}")


def _checked_fit_options(train_path: Path, val_path: Path | None, output_path: Path | None, ckpt_path: Path | None, epochs: int,
                         batch_size: int, lr: float, *, min_batch: int, batch_note: str, suffix: str) -> Path:
    """What `finetune` and `train` refuse alike, before a model is built or a GPU touched; returns the output directory."""
    if epochs < 1:
        raise typer.BadParameter("--epochs must be >= 1")
    if not min_batch <= batch_size <= 65535:
        raise typer.BadParameter(f"--batch-size must be {min_batch} ... 65535{batch_note}")
    if not lr > 0:
        raise typer.BadParameter("--lr must be > 0")
    for f in (train_path, val_path):
        if f is not None and f.suffix != ".parquet":
            raise typer.BadParameter(f"{f} is not in Parquet format")
        if f is not None and not f.is_file():
            raise typer.BadParameter(f"{f}: no such file")
    if ckpt_path is not None and not ckpt_path.is_file():
        raise typer.BadParameter(f"--ckpt {ckpt_path}: no such file")
    return output_path if output_path is not None else train_path.with_suffix(suffix)


@app.command()
def finetune(
    train_path: Path = typer.Argument(..., help="Labelled reads (parquet; ids end in |0 or |1)"),
    val_path: Path | None = typer.Option(None, "--val", help="Validation reads (parquet); without it the training file is split "
                                         "70 / 20 / 10 percent as the reference does and the middle slice validates"),
    output_path: Path | None = typer.Option(None, "--output", "-o", help="Output directory (default: TRAIN with suffix .finetune)"),
    epochs: int = typer.Option(10, "--epochs", help="Epochs"),
    lr: float = typer.Option(1e-4, "--lr", help="AdamW learning rate (weight decay 0.01; ReduceLROnPlateau on val/loss)"),
    batch_size: int = typer.Option(16, "--batch-size", "-b", help="Reads per optimizer step"),
    precision: str = typer.Option("fp16x3", "--precision", help="arithmetic of the frozen backbone: fp16x3 (default) | fp32"),
    seed: int = typer.Option(12345, "--seed", help="Seed of the per-epoch shuffle and of the head's dropout"),
    ckpt_path: Path | None = typer.Option(None, "--ckpt", "-c", help="Path to the checkpoint file to start from"),
    weights: str = typer.Option("yangliz5/chimeralm", "--weights", help="Directory/file with model.safetensors to start from"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose output"),
    train_backbone: bool = typer.Option(False, "--train-backbone", help="Train the backbone together with the head (the reference's "
                                        "freeze_backbone=False): every parameter, in exact fp32; --precision then only names the "
                                        "arithmetic of the validation forwards"),
    hyena_core: str = typer.Option("engine", "--hyena-core", help="With --train-backbone, the Hyena operator's core: engine (the HIP "
                                   "op; reads beyond 8,193 tokens take torch) | torch (conv1d and rfft / irfft)"),
    hyena_long_core: str = typer.Option("torch", "--hyena-long-core", help="With --train-backbone and --hyena-core engine, the core of "
                                        "reads of 8,194 to 32,769 tokens: torch | engine (the segmented HIP op)"),
):
    """Fine-tune the classifier head on labelled reads with the backbone frozen, or with --train-backbone the whole net (writes
    model.safetensors and metrics.tsv)."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s")
    from .headtrain import TRAIN_PRECISIONS

    if hyena_core not in ("engine", "torch"):
        raise typer.BadParameter("--hyena-core must be engine or torch")
    if hyena_long_core not in ("torch", "engine"):
        raise typer.BadParameter("--hyena-long-core must be torch or engine")

    if precision not in TRAIN_PRECISIONS:
        raise typer.BadParameter("--precision must be fp16x3 or fp32: the head trains on the rows of the exact kernels")
    if ckpt_path is not None and weights != "yangliz5/chimeralm":
        raise typer.BadParameter("--ckpt and --weights exclude each other: the fit starts from one set of weights")
    output_path = _checked_fit_options(train_path, val_path, output_path, ckpt_path, epochs, batch_size, lr, min_batch=1, batch_note="",
                                       suffix=".finetune")

    from . import headtrain, lm
    from .fit import split_rows

    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    kw = dict(precision=precision, selfcheck=False, freeze_backbone=True)
    if train_backbone:
        kw = dict(precision=precision, selfcheck=False, freeze_backbone=False, trainable=True, hyena_core=hyena_core,
                  hyena_long_core=hyena_long_core)
    if ckpt_path is not None:
        log.info(f"Loading model from {ckpt_path}")
        model = lm.ChimeraLM.new(**kw).load_reference_checkpoint(ckpt_path)
    else:
        log.info(f"Loading model weights {weights}")
        model = lm.ChimeraLM.from_pretrained(weights, **kw)
    model.to(device)
    train_rows, val_rows = split_rows(train_path, val_path)
    if train_backbone:
        from .hyenatrain import fit_hyena

        hist = fit_hyena(model, train_rows, val_rows, output_path, epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device)
    else:
        hist = headtrain.fit_head(model, train_rows, val_rows, output_path, epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device)
    log.info(f"{len(hist)} epochs; best val/f1 {hist[-1]['val/f1_best']:.4f}; model.safetensors and metrics.tsv saved to {output_path}")


TRAIN_NETS = ("cnn", "mamba", "mambasp")              # `train --net`: the nets whose layers train on engine kernels of their own ...
TRAIN_NET_CHOICES = TRAIN_NETS + ("transformer",)     # ... and the one that trains in torch around the engine's attention core


@app.command()
def train(
    train_path: Path = typer.Argument(..., help="Labelled reads (parquet; ids end in |0 or |1)"),
    val_path: Path | None = typer.Option(None, "--val", help="Validation reads (parquet); without it the training file is split "
                                         "70 / 20 / 10 percent as the reference does and the middle slice validates"),
    output_path: Path | None = typer.Option(None, "--output", "-o", help="Output directory (default: TRAIN with suffix .train)"),
    epochs: int = typer.Option(10, "--epochs", help="Epochs"),
    lr: float = typer.Option(1e-4, "--lr", help="Adam learning rate (ReduceLROnPlateau on val/loss)"),
    batch_size: int = typer.Option(8, "--batch-size", "-b", help="Reads per optimizer step (BatchNorm couples them: never split)"),
    seed: int = typer.Option(12345, "--seed", help="Seed of the initial weights, the per-epoch shuffle and the dropout masks"),
    ckpt_path: Path | None = typer.Option(None, "--ckpt", "-c", help="Path to a DNAConvNet checkpoint to start from (default: "
                                          "torch's initialisation under --seed)"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose output"),
    net: str = typer.Option("cnn", "--net", help="The net to train: cnn (DNAConvNet), mamba or mambasp (configs/model/NET.yaml; the "
                            "Mamba nets take batches of one read too) or transformer (SequenceCNNTransformer; --ckpt starts from a "
                            "reference checkpoint)"),
):
    """Train DNAConvNet (configs/model/cnn.yaml) on labelled reads (writes model.safetensors and metrics.tsv)."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s")
    if net not in TRAIN_NET_CHOICES:
        raise typer.BadParameter(f"--net must be one of {', '.join(TRAIN_NET_CHOICES)}")
    output_path = _checked_fit_options(train_path, val_path, output_path, ckpt_path, epochs, batch_size, lr, min_batch=2 if net == "cnn" else 1,
                                       batch_note=": BatchNorm needs two reads" if net == "cnn" else "", suffix=".train")

    from . import cnntrain, mambatrain, tftrain
    from .config import compose, instantiate
    from .fit import split_rows

    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(seed)                                  # the initial weights
    cfg = compose(Path(__file__).resolve().parent.parent / "configs", "eval.yaml", ["ckpt_path=unused", f"model={net}"], output_dir=output_path)
    model = instantiate(cfg.model, net=instantiate(cfg.model.net, trainable=True))
    if ckpt_path is not None:
        log.info(f"Loading model from {ckpt_path}")
        model.load_reference_checkpoint(ckpt_path)
    model.to(device)
    train_rows, val_rows = split_rows(train_path, val_path)
    fit = {"cnn": cnntrain.fit_cnn, "mamba": mambatrain.fit_mamba, "mambasp": mambatrain.fit_mamba, "transformer": tftrain.fit_transformer}[net]
    hist = fit(model, train_rows, val_rows, output_path, epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device)
    log.info(f"{len(hist)} epochs; best val/f1 {hist[-1]['val/f1_best']:.4f}; model.safetensors and metrics.tsv saved to {output_path}")


@app.command()
def filter(  # noqa: A001 - reference command name
    bam_path: Path = typer.Argument(..., help="Path to the BAM file"),
    predictions_path: Path = typer.Argument(..., help="Path to the predictions file"),
    output_prediction: bool = typer.Option(False, "--output-prediction", "-p", help="write summary of the predictions"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose output"),
):
    """Filter the BAM file by predictions."""
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO, format="%(message)s")
    from .filter import filter_bam_by_predcition

    log.info(f"Filtering {bam_path} by predictions from {predictions_path}")
    res = filter_bam_by_predcition(bam_path, predictions_path, index=True, output_prediction=output_prediction)
    if res:
        log.info(f"kept {res['kept']} records, dropped {res['dropped']}: {res['sorted'] or res['filtered']}")


if __name__ == "__main__":
    app()
