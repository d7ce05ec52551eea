"""In-silico mutagenesis behind the `clm_explain_*` C ABI (csrc/explain.hip): per-base importance of one read, for any net.

The reference's `Mamba2Analyzer.get_position_importance` (/root/reference/chimeralm/explain/motif.py:64-82) replaces one base by `N`,
runs the model again and reports `|p1(read) - p1(mutant)|` per position: one forward of one read and one `.item()` per position.
`position_importance` builds the mutants on the device in batches (the uint8 rows every net's forward takes), runs the net's own
forward on them, and turns each batch's logits into differences with one small kernel behind it; a last kernel folds the windows into
per-base importance and picks the peaks.  Everything is queued on torch's current stream and this module waits for nothing: the
caller does when it reads the result (`Importance.to_host()` and an event, or `.cpu()`).  A net whose own forward waits -- the Mamba
nets look at their fp16x3 logits for NaN -- still does.

Difference kept on purpose: the reference feeds `ord(c)` per character and no `[SEP]` to a model trained on
tokenizer ids; here the read is tokenised as `predict` tokenises it (A, C, G, T, N = 7 ... 11, one trailing `[SEP]`, truncated to the
tokenizer's maximum length, no pads).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N
from .engine import pinned_copy
from .tokenizer import load_tokenizer_from_hyena_model

SUBSTITUTES = {"N": N.EXPLAIN_SUB_N, "all": N.EXPLAIN_SUB_ALL}
SCORES = ("prob", "gap")
PLAN_DTYPE = np.dtype([("start", "<i4"), ("sub", "<i4"), ("slot", "<i4"), ("reserved", "<i4")])   # struct clm_explain_mutant
_TOKENIZER = "hyenadna-small-32k-seqlen"


class ExplainError(RuntimeError):
    pass


@dataclass(frozen=True)
class Options:
    """The scan's options, validated (`ValueError`): see include/chimeralm_hip.h for their meaning."""
    window: int = 1
    stride: int = 1
    substitute: str = "N"
    score: str = "prob"
    top_k: int = 10

    def __post_init__(self):
        for name in ("window", "stride", "top_k"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if self.window < 1 or not 1 <= self.stride <= self.window:
            raise ValueError(f"window >= 1 and 1 <= stride <= window, got window {self.window}, stride {self.stride}")
        if self.substitute not in SUBSTITUTES:
            raise ValueError(f"substitute must be one of {sorted(SUBSTITUTES)}, got {self.substitute!r}")
        if self.substitute == "all" and (self.window, self.stride) != (1, 1):
            raise ValueError("substitute='all' (saturation mutagenesis) needs window = stride = 1")
        if self.score not in SCORES:
            raise ValueError(f"score must be one of {SCORES}, got {self.score!r}")
        if not 1 <= self.top_k <= N.ATTN_MAX_TOP_K:
            raise ValueError(f"top_k must be 1 ... {N.ATTN_MAX_TOP_K}")

    @property
    def n_sub(self) -> int:
        return 4 if self.substitute == "all" else 1


def tokenize(read) -> np.ndarray:
    """uint8 ids of one read as `predict` tokenises it: the bases, then [SEP]; truncated to the tokenizer's maximum length.  A 1-D id
    tensor / array is taken as it is (it must already end in [SEP])."""
    if isinstance(read, str):
        tok = load_tokenizer_from_hyena_model(_TOKENIZER)
        return tok.encode_array(read, tok.max_len_single_sentence)    # (the predict path's max_length, bam.py: 32,768 bases + [SEP])
    ids = read.detach().cpu().numpy() if isinstance(read, torch.Tensor) else np.asarray(read)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError("a read is a sequence string or a 1-D tensor of token ids")
    if ids.size and (ids.min() < 0 or ids.max() > 255):
        raise ValueError("token ids must fit a byte")
    return np.ascontiguousarray(ids.astype(np.uint8))


def build_plan(ids, window: int = 1, stride: int = 1, substitute: str = "N") -> tuple[np.ndarray, int]:
    """The mutants of a tokenised read (`clm_explain_plan`; host only, needs no GPU): a structured array of PLAN_DTYPE records
    (window start, substitute id, slot = window * S + column) in window order, and n_windows.  Raises ValueError for bad options, a
    token that is not a base or a read that does not end in [SEP]."""
    Options(window=window, stride=stride, substitute=substitute)
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint8))
    if ids.ndim != 1:
        raise ValueError("ids must be 1-D")
    lib = N.load()
    n_mut, n_win = C.c_int(0), C.c_int(0)
    args = (C.c_void_p(ids.ctypes.data), int(ids.size), int(window), int(stride), SUBSTITUTES[substitute])
    if lib.clm_explain_plan(*args, None, 0, C.byref(n_mut), C.byref(n_win)) != 0:
        raise ValueError(lib.clm_explain_last_error(None).decode())
    plan = np.zeros(n_mut.value, dtype=PLAN_DTYPE)
    if lib.clm_explain_plan(*args, C.c_void_p(plan.ctypes.data), n_mut.value, C.byref(n_mut), C.byref(n_win)) != 0:
        raise ValueError(lib.clm_explain_last_error(None).decode())
    return plan, n_win.value


@dataclass
class Importance:
    """The scan of one read: device tensors, complete when the stream they were queued on reaches them (nothing here synchronises).
    `logits` fp32 [M + 1, 2] (row 0 the unmodified read, then the mutants in plan order), `dp1` / `dgap` fp32 [n_windows, S] (signed,
    mutant minus read), `importance` fp32 [n_bases], `peak_pos` int32 / `peak_val` fp32 [top_k] (-1 / 0 in empty slots),
    `n_nonfinite` int32 [1]."""
    options: Options
    n_bases: int
    logits: torch.Tensor
    dp1: torch.Tensor
    dgap: torch.Tensor
    importance: torch.Tensor
    peak_pos: torch.Tensor
    peak_val: torch.Tensor
    n_nonfinite: torch.Tensor

    def tensors(self) -> dict[str, torch.Tensor]:
        return {k: getattr(self, k) for k in ("logits", "dp1", "dgap", "importance", "peak_pos", "peak_val", "n_nonfinite")}

    def to_host(self, non_blocking: bool = True) -> "Importance":
        """`engine.pinned_copy` of the tensors."""
        return Importance(self.options, self.n_bases, **pinned_copy(self.tensors(), non_blocking))


class Explainer:
    """One `clm_explain_handle` on `device`: the three kernels on torch's current stream.  One read at a time."""

    def __init__(self, device: torch.device | str | int | None = None):
        self._lib = N.load()
        self._h = None
        device = torch.device("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))
        if device.type != "cuda":
            raise ExplainError("the scan runs on an MI355X (torch device type 'cuda' on ROCm) only; there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        if self._lib.clm_explain_create(self.device.index, C.byref(h)) != 0:
            raise ExplainError(self._lib.clm_explain_last_error(None).decode())
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.clm_explain_last_error(self._h).decode()
            raise (ValueError if rc == N.E_INVALID else ExplainError)(msg)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def rows(self, ids: torch.Tensor, window: int, plan: torch.Tensor, m0: int, rows: int, out: torch.Tensor) -> None:
        """Mutants m0 ... m0 + rows - 1 into the first `rows` rows of `out` (uint8 [>= rows, stride], stride a multiple of 16)."""
        self._check(self._lib.clm_explain_rows(self._h, C.c_void_p(ids.data_ptr()), int(ids.numel()), int(window),
                                               C.c_void_p(plan.data_ptr()), int(plan.shape[0]), int(m0), int(rows),
                                               C.c_void_p(out.data_ptr()), int(out.stride(0)), self._stream()))

    def scores(self, batch_logits: torch.Tensor, has_base: bool, plan: torch.Tensor, m0: int, imp: "Importance") -> None:
        self._check(self._lib.clm_explain_scores(self._h, C.c_void_p(batch_logits.data_ptr()), int(batch_logits.shape[0]), int(has_base),
                                                 C.c_void_p(plan.data_ptr()), int(plan.shape[0]), int(m0), int(imp.dp1.numel()),
                                                 C.c_void_p(imp.logits.data_ptr()), C.c_void_p(imp.dp1.data_ptr()),
                                                 C.c_void_p(imp.dgap.data_ptr()), C.c_void_p(imp.n_nonfinite.data_ptr()), self._stream()))

    def reduce(self, d: torch.Tensor, n_bases: int, window: int, stride: int, top_k: int, importance: torch.Tensor,
               peak_pos: torch.Tensor, peak_val: torch.Tensor) -> None:
        """importance [n_bases] and the top_k peaks from d fp32 [n_windows, S] (contiguous)."""
        self._check(self._lib.clm_explain_reduce(self._h, C.c_void_p(d.data_ptr()), int(n_bases), int(window), int(stride),
                                                 int(d.shape[1]), int(top_k), C.c_void_p(importance.data_ptr()),
                                                 C.c_void_p(peak_pos.data_ptr()), C.c_void_p(peak_val.data_ptr()), self._stream()))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.clm_explain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_explainers: dict = {}


def _explainer(device: torch.device) -> Explainer:
    if device not in _explainers:
        _explainers[device] = Explainer(device)
    return _explainers[device]


def position_importance(net_or_module, read, *, window: int = 1, stride: int = 1, substitute: str = "N", score: str = "prob",
                        top_k: int = 10, batch_size: int = 256, device: torch.device | None = None) -> Importance:
    """Per-base importance of `read` (a sequence string or a 1-D tensor of token ids ending in [SEP]) under `net_or_module` -- a net
    (`forward(input_ids, second=None) -> logits [B, 2]`) or a `ClassificationLit` around one.  The mutants go through the net's own
    forward `batch_size` rows at a time (the first batch carries the unmodified read in row 0; the last one is ragged).  Runs on
    torch's current stream of `device` (default: the id tensor's device if it is on a GPU, else the current one); does not wait."""
    opt = Options(window=window, stride=stride, substitute=substitute, score=score, top_k=top_k)
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 1 <= batch_size <= 65535:
        raise ValueError(f"batch_size must be 1 ... 65535, got {batch_size!r}")
    ids_host = tokenize(read)
    plan_host, n_windows = build_plan(ids_host, window, stride, substitute)
    if device is None:
        device = read.device if isinstance(read, torch.Tensor) and read.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    ex = _explainer(torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device()))
    device = ex.device
    L, n_bases, M, S = int(ids_host.size), int(ids_host.size) - 1, int(plan_host.shape[0]), opt.n_sub

    # the read and its plan cross PCIe once, from page-locked memory (torch's caching host allocator keeps it until the copy is done)
    ids = torch.from_numpy(ids_host).pin_memory().to(device, non_blocking=True)
    plan = torch.from_numpy(plan_host.view(np.int32).reshape(M, 4)).pin_memory().to(device, non_blocking=True)
    f32 = dict(dtype=torch.float32, device=device)
    imp = Importance(opt, n_bases, torch.empty((M + 1, 2), **f32), torch.empty((n_windows, S), **f32), torch.empty((n_windows, S), **f32),
                     torch.empty((n_bases,), **f32), torch.empty((top_k,), dtype=torch.int32, device=device),
                     torch.empty((top_k,), **f32), torch.empty((1,), dtype=torch.int32, device=device))
    stride16 = (L + 15) // 16 * 16
    buf = torch.empty((min(batch_size, M + 1), stride16), dtype=torch.uint8, device=device)   # one buffer: batches are stream-ordered
    net = net_or_module
    with torch.inference_mode():
        buf[0, :L].copy_(ids)
        m0, has_base = 0, 1
        while m0 < M or has_base:
            rows = min(batch_size - has_base, M - m0)
            if rows:
                ex.rows(ids, window, plan, m0, rows, buf[has_base:])
            logits = net(buf[: rows + has_base, :L], None)
            if logits.dtype != torch.float32 or tuple(logits.shape) != (rows + has_base, 2) or not logits.is_contiguous():
                raise ExplainError(f"the net returned {logits.dtype} {tuple(logits.shape)}, expected contiguous fp32 "
                                   f"{(rows + has_base, 2)}")
            ex.scores(logits, bool(has_base), plan, m0, imp)
            m0 += rows
            has_base = 0
        ex.reduce(imp.dp1 if score == "prob" else imp.dgap, n_bases, window, stride, top_k, imp.importance, imp.peak_pos, imp.peak_val)
    return imp
