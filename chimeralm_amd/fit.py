"""The one training loop of the five fit paths (`headtrain.fit_head`, `cnntrain.fit_cnn`, `mambatrain.fit_mamba`,
`tftrain.fit_transformer`, `hyenatrain.fit_hyena`) and the utilities around it: the seeded per-epoch order, the labelled rows of a
parquet file, the best-epoch checkpoint and metrics.tsv.  The paths differ in their training step (`whole_batch_step` or
`micro_batch_step`), in the parameters they optimise and in what they seed; everything else is `fit`.
"""
from __future__ import annotations

import logging
import time
from pathlib import Path

import torch
import torch.nn.functional as F

log = logging.getLogger("chimeralm_amd")
METRIC_COLUMNS = ("epoch", "train/loss", "train/f1", "val/loss", "val/f1", "lr", "seconds")
SHARED_SINE_ALIASES = (".implicit_filter.3.freq", ".implicit_filter.5.freq")   # one module registered three times: .1.freq stays


def epoch_order(n: int, seed: int, epoch: int) -> list[int]:
    """The order the n training rows are visited in epoch `epoch`: a function of (seed, epoch) alone."""
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(n, generator=g).tolist()


def micro_loss(logits: torch.Tensor, labels: torch.Tensor, batch_reads: int) -> torch.Tensor:
    """A micro-batch's share of the batch's mean cross-entropy: the shares of a batch's micro-batches sum to it."""
    return F.cross_entropy(logits, labels, reduction="sum") / batch_reads


def save_checkpoint(model, out_dir: str | Path) -> Path:
    """The model's full state_dict as `model.safetensors` with the reference's keys; the two aliases of the shared sine module are
    left out, as in the released file (`load_reference_checkpoint` restores them from `.1.freq`)."""
    from safetensors.torch import save_file

    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    sd = {k: v.detach().to("cpu").contiguous().clone() for k, v in model.state_dict().items() if not k.endswith(SHARED_SINE_ALIASES)}
    path = out_dir / "model.safetensors"
    save_file(sd, str(path))
    return path


def _f1(tp: float, fp: float, fn: float) -> float:
    return 2.0 * tp / (2.0 * tp + fp + fn) if (2.0 * tp + fp + fn) else 0.0


def _load_reads(rows, tokenizer) -> list[dict]:
    from . import fq
    from .tokenizer import tokenize_and_align_labels_and_quals

    path, start, stop = rows
    feats = [tokenize_and_align_labels_and_quals(rec, tokenizer, tokenizer.max_len_single_sentence) for rec in fq.iter_rows(path, start, stop)]
    bad = [i for i, f in enumerate(feats) if f["labels"] not in (0, 1)]
    if bad:
        raise ValueError(f"{path}: {len(bad)} reads carry no '|0' / '|1' label (first: row {start + bad[0]}); the fine-tune needs labelled reads")
    if not feats:
        raise ValueError(f"{path}: rows [{start}, {stop}) hold no reads")
    return feats


def split_rows(train_path, val_path=None, split=(0.7, 0.2, 0.1)) -> tuple[tuple, tuple]:
    """(train rows, val rows) as (file, first, one past last): a validation file whole, or the reference's percent slices of the
    training file (fq.py:195-217: 70 / 20 / 10; the test tail is left alone)."""
    from . import fq

    n = fq.DataModule._num_rows(train_path)
    if val_path is not None:
        return (str(train_path), 0, n), (str(val_path), 0, fq.DataModule._num_rows(val_path))
    a, b = int(100 * split[0]), int(100 * split[1])
    return (str(train_path), 0, fq.percent_to_row(a, n)), (str(train_path), fq.percent_to_row(a, n), fq.percent_to_row(a + b, n))


def trainable_parameters(module: torch.nn.Module, what: str) -> list[torch.nn.Parameter]:
    """The parameters of `module` (`what`: "net" or "head") an optimizer is to move; raises if there is none."""
    params = [p for p in module.parameters() if p.requires_grad]
    if not params:
        raise ValueError(f"the {what} has no trainable parameter")
    return params


# ------------------------------------------------------------------------------------------------------------- the two steps
# A training step runs the forwards and backwards of ONE batch (gradients were zeroed; the optimizer steps after it) and yields, per
# forward, (that forward's summed loss as an fp64 scalar, its logits, its labels): the loop adds each to its tallies as it comes.
def whole_batch_step(model, ids: torch.Tensor, labels: torch.Tensor):
    """The batch at once under `model.criterion` (the CNN, Mamba, transformer and whole-Hyena fits)."""
    logits = model(ids)
    loss = model.criterion(logits, labels.long().view(-1))
    loss.backward()
    yield loss.detach().double() * len(ids), logits, labels


def micro_batch_step(model, ids: torch.Tensor, labels: torch.Tensor):
    """The batch in micro-batches of what the net's engine runs as one chunk (`net.micro_reads`; a net without an engine: its
    `chunk_reads`, failing that the whole batch), each a `micro_loss` share of the batch's mean cross-entropy: gradients accumulate,
    and a micro-batch's backward comes before the next one's forward (the head fit)."""
    net = model.net
    B, L = ids.shape
    step = net.micro_reads(L, ids.device) if hasattr(net, "micro_reads") else int(getattr(net, "chunk_reads", B))
    for b0 in range(0, B, step):
        logits = model(ids[b0:b0 + step])
        loss = micro_loss(logits, labels[b0:b0 + step], B)
        loss.backward()
        yield loss.detach().double() * B, logits, labels[b0:b0 + step]


# ------------------------------------------------------------------------------------------------------------- the loop
def fit(model, train_rows, val_rows, out_dir, *, params, step, min_reads: int, config: str, epochs: int, batch_size: int, lr: float | None,
        seed: int, device: torch.device | str, tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train `params` of `model` (a `ClassificationLit`) on one GPU.

    Per epoch: the training rows in `epoch_order(n, seed, epoch)`, batches of `batch_size`, one optimizer step per batch around
    `step(model, ids, labels)` (a last batch of fewer than `min_reads` reads is skipped: 2 where BatchNorm needs batch statistics,
    else 1: none is); then validation in file order, in eval mode through the inference kernels, into `EvalMetrics` (or
    `metrics_factory()`: an object with its update / read / close), `scheduler.step(val/loss)`.  Optimizer and scheduler are the
    model's factories (`config` names where they come from) over `params`; `lr` overrides the rate.  A net with a
    `dropout_generator` gets one of its own, seeded with `seed` on `device`.
    `train/loss` is the mean over the epoch's trained reads of the loss each had when its batch was run (a last batch of one read
    counts as one read, not as a batch), `val/loss` the reference's mean of the validation batches' means.
    Writes `out_dir/metrics.tsv` (one row per epoch: METRIC_COLUMNS) and, for the epoch of the best `val/f1` (ties: the earlier),
    `out_dir/model.safetensors`; on return the model holds that epoch's weights too.  Returns the rows of metrics.tsv as dicts, with
    `val/f1_best`."""
    from .tokenizer import DataCollator, load_tokenizer_from_hyena_model

    device = torch.device(device)
    tok = tokenizer if tokenizer is not None else load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    collate = DataCollator(tok).torch_call
    train, val = _load_reads(train_rows, tok), _load_reads(val_rows, tok)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    if model.optimizer_factory is None:
        raise ValueError(f"the model has no optimizer factory ({config}: optimizer)")
    opt = model.optimizer_factory(params=params)
    if lr is not None:
        for g in opt.param_groups:
            g["lr"] = float(lr)
    sched = model.scheduler_factory(optimizer=opt) if model.scheduler_factory is not None else None
    if hasattr(model.net, "dropout_generator"):              # the dropout masks: a generator of the net's own, seeded here
        model.net.dropout_generator = torch.Generator(device=device).manual_seed(int(seed))
    if metrics_factory is None:                              # (a parameter so that a stub net on CPU tensors can bring its own sums)
        from .eval_metrics import EvalMetrics

        metrics_factory = lambda: EvalMetrics(device, n_classes=2, ignore_index=-100)   # noqa: E731
    history, best = [], -1.0
    with (out_dir / "metrics.tsv").open("w") as tsv:
        tsv.write("\t".join(METRIC_COLUMNS) + "\n")
        for epoch in range(epochs):
            t0 = time.perf_counter()
            model.train()
            order = epoch_order(len(train), seed, epoch)
            loss_sum = torch.zeros((), dtype=torch.float64, device=device)
            counts = torch.zeros(3, dtype=torch.float64, device=device)      # tp, fp, fn of the training predictions
            seen = 0
            for i0 in range(0, len(order), batch_size):
                rows = order[i0:i0 + batch_size]
                if len(rows) < min_reads:
                    continue
                batch = collate([train[i] for i in rows])
                opt.zero_grad(set_to_none=True)
                for loss, logits, y in step(model, batch["input_ids"].to(device), batch["labels"].to(device)):
                    pred = logits.detach().argmax(dim=-1)
                    loss_sum += loss
                    counts += torch.stack([((pred == 1) & (y == 1)).sum(), ((pred == 1) & (y == 0)).sum(), ((pred == 0) & (y == 1)).sum()]).double()
                opt.step()
                seen += len(rows)
            model.eval()
            sums = metrics_factory()
            try:
                with torch.no_grad():
                    for i0 in range(0, len(val), batch_size):
                        batch = collate(val[i0:i0 + batch_size])
                        sums.update(model(batch["input_ids"].to(device)), batch["labels"].to(device))
                r = sums.read()
            finally:
                sums.close()
            tp, fp, fn = counts.tolist()
            row = {"epoch": epoch, "train/loss": float(loss_sum) / max(seen, 1), "train/f1": _f1(tp, fp, fn),
                   "val/loss": r["sum_batch_mean_loss"] / r["n_batches"], "val/f1": _f1(r["tp"], r["fp"], r["fn"]),
                   "lr": opt.param_groups[0]["lr"]}
            if sched is not None:
                sched.step(row["val/loss"])
            if row["val/f1"] > best:
                best = row["val/f1"]
                save_checkpoint(model, out_dir)
            row["seconds"] = time.perf_counter() - t0
            tsv.write("\t".join(f"{row[c]:.9g}" if isinstance(row[c], float) else str(row[c]) for c in METRIC_COLUMNS) + "\n")
            tsv.flush()
            row["val/f1_best"] = best
            history.append(row)
            log.info("epoch %d: train/loss %.6f train/f1 %.4f val/loss %.6f val/f1 %.4f (best %.4f) lr %.3g  %.1f s", epoch,
                     row["train/loss"], row["train/f1"], row["val/loss"], row["val/f1"], best, row["lr"], row["seconds"])
    model.load_reference_checkpoint(out_dir / "model.safetensors")       # the model in memory is the one on disk: the best epoch's
    return history
