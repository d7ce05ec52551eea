"""Fine-tune the Hyena head on labelled reads with the backbone frozen (the reference's `HyenaDna(freeze_backbone=True)` under
`train.py`; /root/reference/chimeralm/models/components/hyena.py:218-256, basic_module.py `training_step`).

The backbone runs in the engine exactly as in inference and leaves the final residual rows on the device (`Engine.rows`).  The one
part of the head that sees L tokens per read, the attention pooling, runs forward and backward in the engine on the module's CURRENT
`head.attention.{0,2}` parameters (csrc/pool_train.hip, `clm_pool_forward` / `clm_pool_backward`), wrapped here as a
`torch.autograd.Function`; the classifier behind it sees one 256-vector per read and is plain torch on the module's own `nn.Linear`s.

Deliberate difference from the reference: the frozen backbone runs in INFERENCE arithmetic.  The reference leaves the backbone's
embedding dropout (0.1) active while frozen, because `freeze_backbone` only clears `requires_grad`; here no backbone dropout exists
(DESIGN.md).  The head's own dropouts follow `module.training`, as in the reference.
"""
from __future__ import annotations

import logging
import time
from pathlib import Path

import torch
import torch.nn.functional as F

from ._reload import reload_signature

log = logging.getLogger("chimeralm_amd")
TRAIN_PRECISIONS = ("fp32", "fp16x3")                    # the arithmetics whose kernels leave the fp32 rows (clm_rows)
METRIC_COLUMNS = ("epoch", "train/loss", "train/f1", "val/loss", "val/f1", "lr", "seconds")
SHARED_SINE_ALIASES = (".implicit_filter.3.freq", ".implicit_filter.5.freq")   # one module registered three times: .1.freq stays


def check_train_precision(precision: str) -> None:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"the head trains on the rows of the exact kernels: precision must be 'fp32' or 'fp16x3', not {precision!r}")


class AttentionPool(torch.autograd.Function):
    """pooled [B, 256] = attention pooling of `rows` [B, L, 256] under (w1, b1, w2, b2), differentiable in those four.  `generation`
    is `Engine.rows_generation()` at the time the rows were taken from the engine's workspace (None: the caller owns `rows`);
    `backward` raises, before anything is launched, if the engine has run since: stale rows must not be read."""

    @staticmethod
    def forward(ctx, eng, rows, generation, w1, b1, w2, b2):
        w1c, b1c, w2c = w1.detach().contiguous(), b1.detach().contiguous(), w2.detach().contiguous()
        scores, stats, pooled = eng.pool_forward(rows, w1c, b1c, w2c.view(-1), b2.detach().contiguous())
        ctx.eng, ctx.rows, ctx.generation = eng, rows, generation
        ctx.w2_shape, ctx.b2_shape = w2.shape, b2.shape
        ctx.save_for_backward(w1c, b1c, w2c, scores, stats, pooled)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        eng = ctx.eng
        if ctx.generation is not None and eng.rows_generation() != ctx.generation:
            raise RuntimeError("the engine ran another forward (or reloaded its weights) since this graph's forward: the residual rows "
                               "it would differentiate through are gone.  Call backward() before the next forward")
        w1, b1, w2, scores, stats, pooled = ctx.saved_tensors
        d_w1, d_b1, d_w2, d_b2 = eng.pool_backward(ctx.rows, w1, b1, w2.view(-1), scores, stats, pooled, dpooled.contiguous())
        return None, None, None, d_w1, d_b1, d_w2.view(ctx.w2_shape), d_b2.view(ctx.b2_shape)


def train_engine(net, device: torch.device):
    """The module's engine for the frozen-backbone forward: reloaded when a BACKBONE tensor changed, not when the optimizer moved the
    head -- the engine's own copy of the head is not used here (its logits are discarded).  The next inference forward sees the
    full signature differ and reloads everything, as always."""
    sig = reload_signature(net.backbone)
    eng = getattr(net, "_engine", None)
    if eng is None or eng.device != device or getattr(net, "_backbone_sig", None) != sig:
        eng = net.engine(device)
        net._backbone_sig = sig
    return eng


def head_mlp(net, pooled: torch.Tensor) -> torch.Tensor:
    """classifier + output_layer of the reference head (hyena.py:134-146) as the torch modules they are; dropout follows training."""
    head = net.head
    c = head.classifier
    x = c[2](c[1](c[0](pooled)))
    x = c[5](c[4](c[3](x)))
    res = c[6]
    x = res.dropout(res.layers(x)) + x                   # ResidualBlock (hyena.py:160-180)
    return head.output_layer(x)


def differentiable_logits(net, input_ids: torch.Tensor) -> torch.Tensor:
    """logits [B, 2] with a graph to the head's parameters.  The batch goes through the engine in micro-batches of at most one chunk
    of reads; the rows of every micro-batch but the last are copied out of the engine's workspace (the next forward rewrites it),
    the last one's are read in place -- so one `backward()` serves the whole batch, and must come before the next forward."""
    check_train_precision(net.precision)
    if input_ids.device.type != "cuda":
        raise RuntimeError("chimeralm_amd.HyenaDna runs on an MI355X only (move the batch to 'cuda'); there is no CPU forward")
    eng = train_engine(net, input_ids.device)
    B, L = input_ids.shape
    step = eng.chunk_reads_for(L)                        # reads the engine runs as ONE chunk: the micro-batch
    att0, att2 = net.head.attention[0], net.head.attention[2]
    out = []
    for b0 in range(0, B, step):
        eng.forward(input_ids[b0:b0 + step])              # (the engine's own logits -- its copy of the head -- are discarded)
        rows, gen = eng.rows(), eng.rows_generation()
        if b0 + step < B:
            rows, gen = rows.clone(), None
        pooled = AttentionPool.apply(eng, rows, gen, att0.weight, att0.bias, att2.weight, att2.bias)
        out.append(head_mlp(net, pooled))
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)


# ------------------------------------------------------------------------------------------------------------- the loop
def epoch_order(n: int, seed: int, epoch: int) -> list[int]:
    """The order the n training rows are visited in epoch `epoch`: a function of (seed, epoch) alone."""
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(n, generator=g).tolist()


def micro_loss(logits: torch.Tensor, labels: torch.Tensor, batch_reads: int) -> torch.Tensor:
    """A micro-batch's share of the batch's mean cross-entropy: the shares of a batch's micro-batches sum to it."""
    return F.cross_entropy(logits, labels, reduction="sum") / batch_reads


def head_parameters(model) -> list[torch.nn.Parameter]:
    return [p for p in model.net.head.parameters() if p.requires_grad]


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


def fit_head(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 16, lr: float | None = None,
             seed: int = 12345, device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train `model.net.head` (a `ClassificationLit` over `HyenaDna(freeze_backbone=True)`) on one GPU.

    Per epoch: the training rows in `epoch_order(n, seed, epoch)`, batches of `batch_size`, each run as micro-batches of one engine
    chunk whose losses are `micro_loss` shares of the batch's mean cross-entropy (gradients accumulate, one optimizer step per
    batch); then validation in file order through `EvalMetrics` (or `metrics_factory()`: an object with its update / read / close), `scheduler.step(val/loss)`.  Optimizer and scheduler are the model's
    factories (the reference's AdamW 1e-4 / 0.01 and ReduceLROnPlateau) over the head's parameters; `lr` overrides the rate.
    `train/loss` is the mean over the epoch's reads of the loss each had when its batch was run (a last batch of one read counts as
    one read, not as a batch), `val/loss` the reference's mean of the validation batches' means.
    Writes `out_dir/metrics.tsv` (one row per epoch: METRIC_COLUMNS) and, for the epoch of the best `val/f1` (ties: the earlier),
    `out_dir/model.safetensors`; on return the model holds that epoch's weights too.  Returns the rows of metrics.tsv as dicts, with
    `val/f1_best`."""
    from .tokenizer import DataCollator, load_tokenizer_from_hyena_model

    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be >= 1")
    device = torch.device(device)
    net = model.net
    tok = tokenizer if tokenizer is not None else load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    collate = DataCollator(tok).torch_call
    train, val = _load_reads(train_rows, tok), _load_reads(val_rows, tok)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    params = head_parameters(model)
    if not params:
        raise ValueError("the head has no trainable parameter")
    opt = model.optimizer_factory(params=params)
    if lr is not None:
        for g in opt.param_groups:
            g["lr"] = float(lr)
    sched = model.scheduler_factory(optimizer=opt) if model.scheduler_factory is not None else None
    torch.manual_seed(seed)                                   # the head's dropout masks
    if metrics_factory is None:                              # (a parameter so that a stub net on CPU tensors can bring its own sums)
        from .eval_metrics import EvalMetrics

        metrics_factory = lambda: EvalMetrics(device, n_classes=2, ignore_index=-100)   # noqa: E731
    # reads of one micro-batch: what the net's engine runs as one chunk (a net without an engine: its chunk_reads)
    micro = net.micro_reads if hasattr(net, "micro_reads") else (lambda length, dev: int(getattr(net, "chunk_reads", batch_size)))
    history, best = [], -1.0
    with (out_dir / "metrics.tsv").open("w") as tsv:
        tsv.write("\t".join(METRIC_COLUMNS) + "\n")
        for epoch in range(epochs):
            t0 = time.perf_counter()
            model.train()
            order = epoch_order(len(train), seed, epoch)
            loss_sum = torch.zeros((), dtype=torch.float64, device=device)
            counts = torch.zeros(3, dtype=torch.float64, device=device)      # tp, fp, fn of the training predictions
            for i0 in range(0, len(order), batch_size):
                batch = collate([train[i] for i in order[i0:i0 + batch_size]])
                ids, labels = batch["input_ids"].to(device), batch["labels"].to(device)
                B, L = ids.shape
                step = micro(L, device)
                opt.zero_grad(set_to_none=True)
                for b0 in range(0, B, step):                  # forward and backward of a micro-batch before the next one's forward
                    logits = model(ids[b0:b0 + step])
                    loss = micro_loss(logits, labels[b0:b0 + step], B)
                    loss.backward()
                    pred, y = logits.detach().argmax(dim=-1), labels[b0:b0 + step]
                    loss_sum += loss.detach().double() * B   # (the micro-batch's summed loss)
                    counts += torch.stack([((pred == 1) & (y == 1)).sum(), ((pred == 1) & (y == 0)).sum(), ((pred == 0) & (y == 1)).sum()]).double()
                opt.step()
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
            row = {"epoch": epoch, "train/loss": float(loss_sum) / len(order), "train/f1": _f1(tp, fp, fn),
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
