"""Metric sums of the test stage behind the `clm_eval_*` C ABI (csrc/eval_metrics.hip), and the reference's metrics from them.

The reference's `test_step` (/root/reference/chimeralm/models/basic_module.py:153-175) feeds torchmetrics' binary `F1Score`,
`Precision`, `Recall` and a `MeanMetric` of the batch losses on the host, with a sync per batch.  `EvalMetrics.update` queues one
small kernel behind the forward instead; `read` is the one wait of the stage.  `metrics_from_result` restates torchmetrics' binary
definitions (zero-division 0) in double on the host; torchmetrics itself is not a dependency.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N

COUNT_FIELDS = ("tp", "fp", "tn", "fn", "n_valid", "n_ignored", "n_batches", "n_empty_batches", "n_invalid_labels", "n_nonfinite")
SUM_FIELDS = ("sum_batch_mean_loss", "sum_loss")


class EvalError(RuntimeError):
    pass


def result_to_dict(r: N.ClmEvalResult) -> dict:
    return {k: getattr(r, k) for k in COUNT_FIELDS + SUM_FIELDS}


def result_from_dict(d: dict) -> N.ClmEvalResult:
    return N.ClmEvalResult(**{k: d[k] for k in COUNT_FIELDS + SUM_FIELDS})


def _ratio(num: float, den: float) -> float:
    return num / den if den else 0.0


def metrics_from_result(r: dict) -> dict:
    """The reference's four logged names, `test/loss_per_read` and the raw counts.  `test/loss` is the mean of the batches' mean
    losses (MeanMetric weights every batch alike), `test/loss_per_read` the mean over reads."""
    tp, fp, fn = r["tp"], r["fp"], r["fn"]
    out = {"test/loss": _ratio(r["sum_batch_mean_loss"], r["n_batches"]),
           "test/f1": _ratio(2.0 * tp, 2 * tp + fp + fn),
           "test/precision": _ratio(float(tp), tp + fp),
           "test/recall": _ratio(float(tp), tp + fn),
           "test/loss_per_read": _ratio(r["sum_loss"], r["n_valid"])}
    out.update({f"test/{k}": r[k] for k in COUNT_FIELDS})
    return out


class EvalMetrics:
    """One `clm_eval_handle`.  `device=None` is a host-only handle: it needs no GPU and only totals other handles' results."""

    def __init__(self, device: torch.device | None, n_classes: int = 2, ignore_index: int = -100):
        self._lib = N.load()
        self._h = C.c_void_p()
        self.device = device
        dev = -1 if device is None else (device.index if device.index is not None else torch.cuda.current_device())
        if self._lib.clm_eval_create(dev, n_classes, ignore_index, C.byref(self._h)) != 0:
            self._h = None
            raise EvalError(self._lib.clm_eval_last_error(None).decode())

    def _check(self, rc: int):
        if rc != 0:
            raise EvalError(self._lib.clm_eval_last_error(self._h).decode())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device is not None else None

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """Queue one batch on torch's current stream (the one `logits` was produced on); does not wait."""
        if not (logits.is_cuda and labels.is_cuda and logits.dtype == torch.float32 and labels.dtype == torch.int64):
            raise ValueError("update needs fp32 logits [B, 2] and int64 labels [B] on the device")
        if logits.dim() != 2 or logits.shape[1] != 2 or labels.shape != (logits.shape[0],):
            raise ValueError(f"update needs logits [B, 2] and labels [B], got {tuple(logits.shape)} and {tuple(labels.shape)}")
        logits, labels = logits.contiguous(), labels.contiguous()
        self._check(self._lib.clm_eval_update(self._h, C.c_void_p(logits.data_ptr()), C.c_void_p(labels.data_ptr()),
                                              logits.shape[0], self._stream()))

    def read(self) -> dict:
        r = N.ClmEvalResult()
        self._check(self._lib.clm_eval_read(self._h, C.byref(r), self._stream()))
        return result_to_dict(r)

    def merge(self, other: dict) -> None:
        r = result_from_dict(other)
        self._check(self._lib.clm_eval_merge(self._h, C.byref(r)))

    def reset(self) -> None:
        self._check(self._lib.clm_eval_reset(self._h, self._stream()))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.clm_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_results(results: list[dict], ignore_index: int = -100) -> dict:
    """The total of the ranks' results, added in list (rank) order: every rank that does this gets the same bits."""
    total = EvalMetrics(None, ignore_index=ignore_index)
    try:
        for r in results:
            total.merge(r)
        return total.read()
    finally:
        total.close()
