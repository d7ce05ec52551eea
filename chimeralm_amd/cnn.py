"""Drop-in for the reference's third net, `DNAConvNet` (/root/reference/chimeralm/models/components/cnn.py, configs/model/cnn.yaml),
with the forward on MI355X.

Same constructor arguments, same `state_dict()` keys (torch's own modules are the parameter containers, so
`conv_blocks.{i}.0.weight`, `conv_blocks.{i}.1.running_var`, `fc.1.num_batches_tracked` etc. come out exactly as in the reference),
same `forward(input_ids, input_quals=None) -> logits [B, 2]` (eval mode: BatchNorm on its running statistics, dropout off) and the
`number_of_classes` attribute `ClassificationLit` reads.  The arithmetic runs in csrc/cnn.hip + csrc/tail32.hip behind the
`clm_cnn_*` C ABI; there is no CPU path.  Reads must have at least 64 tokens (three max-pools of 4), as in the reference.  Token ids
outside [0, 12) are clamped into the table (the reference's nn.Embedding raises instead).

Engine knob absent in the reference: `precision` -- "fp16x3" (the default: blocks 1 and 2, 97 % of the FLOPs, as three fp16 MFMAs
on hi + lo halfs per product) or "fp32" (the exact-fp32 MFMA).  fp16x3 packs weights x 2^10 as fp16 halfs, which saturates for
|w| >= 64: if any conv or fc weight is that large, the module runs the exact-fp32 kernels instead, records it in
`precision_report` and logs a warning.

Training (`trainable=True`, keyword-only, absent in the reference, where every net trains): in `train()` mode with autograd on, the
forward runs on batch statistics with a graph to every parameter (cnntrain.py, csrc/cnn_train.hip: exact fp32, dropout masks from
`torch.rand` on `dropout_generator`) and updates the running statistics.  Everything else -- `trainable=False`, `eval()`, `no_grad`
-- is the inference forward above, unchanged.
"""
from __future__ import annotations

import ctypes as C
from functools import partial

import numpy as np
import torch
from torch import nn

from . import _native as N
from ._guard import x3_range_report
from ._reload import reload_signature
from .engine import IDS_DT

PRODUCTION = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                  hidden_dim=512, number_of_classes=2, padding_idx=4)


class CnnEngineError(RuntimeError):
    pass


class DNAConvNet(nn.Module):
    def __init__(self, vocab_size: int, embedding_dim: int, num_filters: list[int], kernel_sizes: list[int], pool_sizes: list[int],
                 hidden_dim: int, number_of_classes: int = 2, dropout: float = 0.1, padding_idx: int = 4, *,
                 precision: str = "fp16x3", trainable: bool = False):
        super().__init__()
        got = dict(vocab_size=vocab_size, embedding_dim=embedding_dim, num_filters=list(num_filters), kernel_sizes=list(kernel_sizes),
                   pool_sizes=list(pool_sizes), hidden_dim=hidden_dim, number_of_classes=number_of_classes, padding_idx=padding_idx)
        if got != PRODUCTION:
            raise NotImplementedError("the MI355X DNAConvNet implements the production shape: vocab 12, embedding 256, filters "
                                      "[256, 256, 256], kernels [7, 7, 7], pools [4, 4, 4], hidden 512, 2 classes, padding_idx 4 "
                                      "(configs/model/cnn.yaml)")
        if precision not in ("fp32", "fp16x3"):
            raise ValueError("precision must be fp32 (exact fp32 products) or fp16x3 (every operand of blocks 1 and 2 as two halfs, "
                             "three fp16 MFMAs per product: fp32-class logits)")
        self.number_of_classes, self.precision = number_of_classes, precision
        self.precision_report: dict = {}
        self.embedding = nn.Embedding(vocab_size, embedding_dim, padding_idx=padding_idx)
        self.conv_blocks = nn.ModuleList()
        cin = embedding_dim
        for f, k, p in zip(num_filters, kernel_sizes, pool_sizes):
            self.conv_blocks.append(nn.Sequential(nn.Conv1d(cin, f, k, padding="same"), nn.BatchNorm1d(f), nn.GELU(), nn.MaxPool1d(p),
                                                  nn.Dropout(dropout)))
            cin = f
        self.adaptive_pool = nn.AdaptiveAvgPool1d(1)
        self.fc = nn.Sequential(nn.Linear(num_filters[-1], hidden_dim), nn.BatchNorm1d(hidden_dim), nn.GELU(), nn.Dropout(dropout),
                                nn.Linear(hidden_dim, number_of_classes))
        self._h, self._dev, self._sig, self._hprec = None, None, None, None
        self.trainable, self.dropout = bool(trainable), float(dropout)
        self.dropout_generator: torch.Generator | None = None   # None: the device's default generator (torch.manual_seed)
        self.last_dropout_masks = None                          # the keep masks of the last training forward (None at dropout 0)
        self.last_batch_stats = None                            # its batch means and biased variances, [3, 256] each
        self.train_workspace_limit: int | None = None           # bytes a training batch's workspace may take (None: the engine's default)
        self._train = None

    # ------------------------------------------------------------------ engine plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise CnnEngineError(N.load().clm_cnn_last_error(self._h).decode())

    def _arith(self) -> str:
        """The arithmetic the loaded weights allow: fp16x3 only while every conv / fc weight is inside its packing's range."""
        ws = [b[0].weight for b in self.conv_blocks] + [self.fc[0].weight, self.fc[4].weight]
        self.precision_report = x3_range_report("DNAConvNet", self.precision, ws)
        return self.precision_report.get("fallback_precision", self.precision)

    def _prepare(self, device: torch.device):
        # (not `_engine`: predict.py's end-of-run device check reads `net._engine` as the Hyena engine object)
        lib = N.load()
        sig = reload_signature(self)
        if self._h is not None and self._dev == device and sig == self._sig:
            return lib
        prec = self._arith()
        if self._h is None or self._dev != device or self._hprec != prec:
            self.close()
            h = C.c_void_p()
            dev = device.index if device.index is not None else torch.cuda.current_device()
            if lib.clm_cnn_create(dev, N.PRECISIONS[prec], C.byref(h)) != 0:
                raise CnnEngineError(lib.clm_cnn_last_error(None).decode())
            self._h, self._dev, self._hprec = h, device, prec
        items = [(k, t) for k, t in self.state_dict().items() if not k.endswith("num_batches_tracked")]
        N.upload_state_dict(items, partial(lib.clm_cnn_load_weight, self._h), self._check)   # weights replaced or modified in place -> reload
        self._check(lib.clm_cnn_finalize(self._h))
        self._sig = sig
        return lib

    def refresh_weights(self) -> None:
        """The next forward reloads the engine from this module's tensors: for edits the signature cannot see (`p.data.mul_()`)."""
        self._sig = None

    def forward(self, input_ids: torch.Tensor, input_quals: torch.Tensor | None = None) -> torch.Tensor:
        """`input_quals` is accepted and ignored, as in the reference."""
        if input_ids.device.type != "cuda":
            raise RuntimeError("chimeralm_amd.DNAConvNet runs on an MI355X only; there is no CPU forward")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32, torch.uint8):
            raise ValueError("input_ids must be [batch, length] of int64 / int32 / uint8")
        if input_ids.stride(1) != 1:
            input_ids = input_ids.contiguous()
        if self.trainable and self.training and torch.is_grad_enabled():
            from .cnntrain import train_forward

            return train_forward(self, input_ids)
        lib = self._prepare(input_ids.device)
        B, L = input_ids.shape
        out = torch.empty((B, self.number_of_classes), dtype=torch.float32, device=input_ids.device)
        self._check(lib.clm_cnn_forward(self._h, C.c_void_p(input_ids.data_ptr()), IDS_DT[input_ids.dtype], input_ids.stride(0), B, L,
                                        C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(input_ids.device).cuda_stream)))
        return out

    def debug_fetch(self, name: str, shape) -> np.ndarray:
        """Intermediates of the last forward: "block0" [B, L/4, 256], "block1" [B, L/16, 256], "partial" [B, ceil((L/64) / 16), 256]
        (block 2's pooled rows summed per tile of 16), "pooled" [B, 256]."""
        arr = np.empty(shape, dtype=np.float32)
        self._check(N.load().clm_cnn_debug_fetch(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def train_engine(self, device: torch.device):
        """The module's training engine on `device` (cnntrain.CnnTrainEngine), made on first use."""
        from .cnntrain import CnnTrainEngine

        if self._train is None or self._train.device != device or self._train.workspace_limit != self.train_workspace_limit:
            if self._train is not None:
                self._train.close()
            self._train = CnnTrainEngine(device, self.train_workspace_limit)
        return self._train

    def close(self):
        if getattr(self, "_train", None) is not None:
            self._train.close()
            self._train = None
        if getattr(self, "_h", None) is not None:
            N.load().clm_cnn_destroy(self._h)
            self._h = None
            self._sig = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
