"""Train DNAConvNet on one MI355X (the reference's `train.py` with `model=cnn`, its own default; the reference's
chimeralm/models/components/cnn.py in `train()`, basic_module.py `training_step`).

The three convolution blocks and the mean over positions run forward (on batch statistics) and backward in the engine on the
module's CURRENT parameters (csrc/cnn_train.hip, `clm_cnn_train_*`), wrapped here as a `torch.autograd.Function`; `fc` sees one
256-vector per read and is plain torch on the module's own layers.  BatchNorm couples the reads of a batch, so a batch is never split
into micro-batches: one whose workspace does not fit is refused.

Deliberate differences from the reference: the dropout masks are drawn by `torch.rand` in the engine's token-major layout
-- seeded and reproducible, but not the reference's random stream -- and the training arithmetic is exact fp32 whatever the module's
inference `precision`.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from pathlib import Path

import numpy as np
import torch

from . import _native as N
from .engine import IDS_DT

log = logging.getLogger("chimeralm_amd")
N_PARAMS = 13                                # embedding, then (W, b, g, beta) of blocks 0, 1, 2: CLM_CNN_TRAIN_PARAMS


class CnnTrainError(RuntimeError):
    pass


def block_lengths(L: int) -> list[int]:
    """L_0 .. L_3: every max-pool floors."""
    out = [int(L)]
    for _ in range(3):
        out.append(out[-1] // 4)
    return out


def engine_parameters(net) -> list[torch.nn.Parameter]:
    """The parameters the engine differentiates, in the ABI's order."""
    ps = [net.embedding.weight]
    for blk in net.conv_blocks:
        ps += [blk[0].weight, blk[0].bias, blk[1].weight, blk[1].bias]
    return ps


class CnnTrainEngine:
    """One `clm_cnn_train_handle`.  `workspace_limit`: bytes a batch's workspace may take (None: the engine's default)."""

    def __init__(self, device: torch.device, workspace_limit: int | None = None):
        self.lib = N.load()
        self.device, self.workspace_limit = device, workspace_limit
        h = C.c_void_p()
        dev = device.index if device.index is not None else torch.cuda.current_device()
        if self.lib.clm_cnn_train_create(dev, int(workspace_limit or 0), C.byref(h)) != 0:
            raise CnnTrainError(self.lib.clm_cnn_train_last_error(None).decode())
        self._h = h
        self.shape = None                    # (B, L) of the last forward

    def _check(self, rc: int):
        if rc != 0:
            raise CnnTrainError(self.lib.clm_cnn_train_last_error(self._h).decode())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def generation(self) -> int:
        return int(self.lib.clm_cnn_train_generation(self._h))

    def forward(self, ids: torch.Tensor, params: list[torch.Tensor], keeps: list[torch.Tensor] | None, scale: float):
        """-> pooled [B, 256], batch means [3, 256], biased batch variances [3, 256], the generation to hand to `backward`."""
        B, L = ids.shape
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != ids.device:
                raise ValueError("the engine trains contiguous fp32 parameters on the batch's device")
        pooled = torch.empty((B, 256), dtype=torch.float32, device=ids.device)
        mean, var = torch.empty((3, 256), dtype=torch.float32, device=ids.device), torch.empty((3, 256), dtype=torch.float32, device=ids.device)
        pp = (C.c_void_p * N_PARAMS)(*[p.data_ptr() for p in params])
        kp = None
        if keeps is not None:
            Ls = block_lengths(L)
            for i, k in enumerate(keeps):
                if k.dtype != torch.uint8 or not k.is_contiguous() or tuple(k.shape) != (B, Ls[i + 1], 256):
                    raise ValueError("keep masks are contiguous uint8 [B, L_{i+1}, 256]")
            kp = (C.c_void_p * 3)(*[k.data_ptr() for k in keeps])
        self._check(self.lib.clm_cnn_train_forward(self._h, C.c_void_p(ids.data_ptr()), IDS_DT[ids.dtype], ids.stride(0), B, L, pp, kp, float(scale),
                                                   C.c_void_p(pooled.data_ptr()), C.c_void_p(mean.data_ptr()), C.c_void_p(var.data_ptr()),
                                                   self._stream()))
        self.shape = (B, L)
        return pooled, mean, var, self.generation()

    def backward(self, generation: int, dpooled: torch.Tensor, like: list[torch.Tensor], out: list[torch.Tensor] | None = None,
                 beta: float = 0.0) -> list[torch.Tensor]:
        """The 13 gradients (shaped like `like`); with `out` and beta = 1 they are added to what `out` holds."""
        grads = [torch.empty_like(p) for p in like] if out is None else out
        gp = (C.c_void_p * N_PARAMS)(*[g.data_ptr() for g in grads])
        self._check(self.lib.clm_cnn_train_backward(self._h, generation, C.c_void_p(dpooled.data_ptr()), gp, float(beta), self._stream()))
        return grads

    def debug_fetch(self, name: str) -> np.ndarray:
        """"z0".."z2", "y0".."y2", "dz0".."dz2" fp32 [B, L_i, 256]; "choice0".."choice2" uint8 [B, L_{i+1}, 256] of the last step."""
        B, L = self.shape
        Ls, i = block_lengths(L), int(name[-1])
        arr = np.empty((B, Ls[i + 1], 256), dtype=np.uint8) if name.startswith("choice") else np.empty((B, Ls[i], 256), dtype=np.float32)
        self._check(self.lib.clm_cnn_train_debug_fetch(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.clm_cnn_train_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CnnBlocks(torch.autograd.Function):
    """(pooled [B, 256], batch means [3, 256], biased batch variances [3, 256]) of `ids` under the 13 engine parameters,
    differentiable in them through `pooled`.  `backward` raises, before anything is launched, if the engine ran another forward
    since: the intermediates it would differentiate through are gone."""

    @staticmethod
    def forward(ctx, eng, ids, keeps, scale, *params):
        det = [p.detach() for p in params]
        pooled, mean, var, gen = eng.forward(ids, det, keeps, scale)
        ctx.eng, ctx.gen, ctx.keeps, ctx.like = eng, gen, keeps, det       # (the masks stay alive until the backward has read them)
        ctx.mark_non_differentiable(mean, var)
        return pooled, mean, var

    @staticmethod
    def backward(ctx, dpooled, _dmean, _dvar):
        eng = ctx.eng
        if eng.generation() != ctx.gen:
            raise RuntimeError("the engine ran another training forward since this graph's forward: the convolution outputs it would "
                               "differentiate through are gone.  Call backward() before the next forward")
        grads = eng.backward(ctx.gen, dpooled.contiguous().float(), ctx.like)
        return (None, None, None, None, *grads)


def train_forward(net, input_ids: torch.Tensor) -> torch.Tensor:
    """logits [B, 2] of `net` (a `DNAConvNet(trainable=True)` in training mode) with a graph to every parameter; updates the running
    statistics as `nn.BatchNorm1d` does.  The masks drawn are left in `net.last_dropout_masks` (None at dropout 0), the blocks' batch
    statistics in `net.last_batch_stats`."""
    B, L = input_ids.shape
    if B < 2:
        raise ValueError(f"training needs a batch of at least 2 reads: BatchNorm's batch statistics (torch raises 'Expected more than 1 "
                         f"value per channel when training'), got {B}")
    dev = input_ids.device
    eng = net.train_engine(dev)
    Ls = block_lengths(L)
    p = float(net.dropout)
    keeps, fc_keep, scale = None, None, 1.0
    if p > 0.0:
        gen = net.dropout_generator
        keeps = [(torch.rand((B, Ls[i + 1], 256), device=dev, generator=gen) >= p).to(torch.uint8) for i in range(3)]
        fc_keep = (torch.rand((B, net.fc[0].out_features), device=dev, generator=gen) >= p).to(torch.float32)
        scale = 1.0 / (1.0 - p)
    net.last_dropout_masks = None if keeps is None else keeps + [fc_keep]
    pooled, mean, var = CnnBlocks.apply(eng, input_ids, keeps, scale, *engine_parameters(net))
    net.last_batch_stats = (mean, var)                    # [3, 256] each: the blocks' batch means and biased variances
    with torch.no_grad():
        for i, blk in enumerate(net.conv_blocks):
            bn, n = blk[1], B * Ls[i]
            m = bn.momentum
            bn.running_mean.mul_(1.0 - m).add_(mean[i], alpha=m)
            bn.running_var.mul_(1.0 - m).add_(var[i], alpha=m * n / (n - 1))
            bn.num_batches_tracked += 1
    fc = net.fc
    h = fc[2](fc[1](fc[0](pooled)))                       # (fc.1 in training mode: batch statistics, its own running update)
    if fc_keep is not None:
        h = h * (fc_keep * scale)
    return fc[4](h)


# ------------------------------------------------------------------------------------------------------------- the loop
def fit_cnn(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 8, lr: float | None = None, seed: int = 12345,
            device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train every parameter of `model.net` (a `ClassificationLit` over `DNAConvNet(trainable=True)`) on one GPU.

    Per epoch: the training rows in `headtrain.epoch_order(n, seed, epoch)`, batches of `batch_size` (the reference's 8), ONE
    optimizer step per batch over all parameters -- a batch is never split, BatchNorm couples its reads; a last batch of one read is
    skipped, as it has no batch statistics -- then validation in file order, in eval mode through the inference kernels, into
    `EvalMetrics` (or `metrics_factory()`), `scheduler.step(val/loss)`.  Optimizer and scheduler are the model's factories (the
    reference's Adam 1e-4 and ReduceLROnPlateau, configs/model/cnn.yaml); `lr` overrides the rate.  Writes `out_dir/metrics.tsv`
    (headtrain.METRIC_COLUMNS) and, for the epoch of the best `val/f1` (ties: the earlier), `out_dir/model.safetensors`; on return the
    model holds that epoch's weights too.  Returns the rows of metrics.tsv as dicts, with `val/f1_best`."""
    if epochs < 1 or batch_size < 2:
        raise ValueError("epochs must be >= 1 and batch_size >= 2 (BatchNorm needs two reads)")
    return fit_all_parameters(model, train_rows, val_rows, out_dir, epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device,
                              tokenizer=tokenizer, metrics_factory=metrics_factory, min_reads=2, config="configs/model/cnn.yaml")


def fit_all_parameters(model, train_rows, val_rows, out_dir, *, epochs: int, batch_size: int, lr: float | None, seed: int,
                       device: torch.device | str, tokenizer, metrics_factory, min_reads: int, config: str) -> list[dict]:
    """The loop of `fit_cnn` and `mambatrain.fit_mamba`: one optimizer step per batch over every parameter of `model.net`, validation
    through the inference kernels, the best-`val/f1` checkpoint and metrics.tsv.  A last batch of fewer than `min_reads` reads is
    skipped (2 where BatchNorm needs batch statistics, else 1: none is)."""
    from .headtrain import METRIC_COLUMNS, _f1, _load_reads, epoch_order, save_checkpoint
    from .tokenizer import DataCollator, load_tokenizer_from_hyena_model

    device = torch.device(device)
    tok = tokenizer if tokenizer is not None else load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    collate = DataCollator(tok).torch_call
    train, val = _load_reads(train_rows, tok), _load_reads(val_rows, tok)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    params = [p for p in model.net.parameters() if p.requires_grad]
    if not params:
        raise ValueError("the net has no trainable parameter")
    if model.optimizer_factory is None:
        raise ValueError(f"the model has no optimizer factory ({config}: optimizer)")
    opt = model.optimizer_factory(params=params)
    if lr is not None:
        for g in opt.param_groups:
            g["lr"] = float(lr)
    sched = model.scheduler_factory(optimizer=opt) if model.scheduler_factory is not None else None
    if hasattr(model.net, "dropout_generator"):              # the dropout masks: a generator of the net's own, seeded here
        model.net.dropout_generator = torch.Generator(device=device).manual_seed(int(seed))
    if metrics_factory is None:
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
                ids, y = batch["input_ids"].to(device), batch["labels"].to(device)
                opt.zero_grad(set_to_none=True)
                logits = model(ids)
                loss = model.criterion(logits, y.long().view(-1))
                loss.backward()
                opt.step()
                pred = logits.detach().argmax(dim=-1)
                loss_sum += loss.detach().double() * len(rows)
                counts += torch.stack([((pred == 1) & (y == 1)).sum(), ((pred == 1) & (y == 0)).sum(), ((pred == 0) & (y == 1)).sum()]).double()
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
