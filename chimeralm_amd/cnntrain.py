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

import numpy as np
import torch

from . import _native as N
from ._trainop import is_plain_fp32, stream_of
from .engine import IDS_DT

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

    def generation(self) -> int:
        return int(self.lib.clm_cnn_train_generation(self._h))

    def forward(self, ids: torch.Tensor, params: list[torch.Tensor], keeps: list[torch.Tensor] | None, scale: float):
        """-> pooled [B, 256], batch means [3, 256], biased batch variances [3, 256], the generation to hand to `backward`."""
        B, L = ids.shape
        if not all(is_plain_fp32(p, ids.device) for p in params):
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
                                                   stream_of(self.device)))
        self.shape = (B, L)
        return pooled, mean, var, self.generation()

    def backward(self, generation: int, dpooled: torch.Tensor, like: list[torch.Tensor], out: list[torch.Tensor] | None = None,
                 beta: float = 0.0) -> list[torch.Tensor]:
        """The 13 gradients (shaped like `like`); with `out` and beta = 1 they are added to what `out` holds."""
        grads = [torch.empty_like(p) for p in like] if out is None else out
        gp = (C.c_void_p * N_PARAMS)(*[g.data_ptr() for g in grads])
        self._check(self.lib.clm_cnn_train_backward(self._h, generation, C.c_void_p(dpooled.data_ptr()), gp, float(beta), stream_of(self.device)))
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
    """Train every parameter of `model.net` (a `ClassificationLit` over `DNAConvNet(trainable=True)`) on one GPU: `fit.fit` with
    `fit.whole_batch_step` at the reference's batch of 8 -- a batch is never split, BatchNorm couples its reads, and a last batch of
    one read is skipped, as it has no batch statistics.  Optimizer and scheduler are the reference's Adam 1e-4 and ReduceLROnPlateau
    (configs/model/cnn.yaml); the dropout masks follow `seed` through `net.dropout_generator`."""
    from . import fit

    if epochs < 1 or batch_size < 2:
        raise ValueError("epochs must be >= 1 and batch_size >= 2 (BatchNorm needs two reads)")
    return fit.fit(model, train_rows, val_rows, out_dir, params=fit.trainable_parameters(model.net, "net"), step=fit.whole_batch_step,
                   min_reads=2, config="configs/model/cnn.yaml", epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device,
                   tokenizer=tokenizer, metrics_factory=metrics_factory)
