"""Reads longer than the model's context, judged in overlapping windows: behind the `clm_longread_*` C ABI (csrc/longread_plan.cpp,
csrc/longread.hip), for any net.

The reference truncates a read to the tokenizer's 32,768 bases (/root/reference/chimeralm/data/bam.py:166-170): a chimera junction
behind them is never seen.  `tiled_forward` takes the UNTRUNCATED left-padded uint8 batch on the device, writes the head batch --
byte for byte the batch the truncating path delivers, so window 0 of every read has today's logits -- and the extra windows of the
long reads with one small kernel, runs the net's own forward on them, and reduces the windows' logits per read with another: the
window with the largest logit1 - logit0 is the read's.  Everything is queued on torch's current stream and nothing here waits (a net
whose own forward waits still does).  The definitions are in include/chimeralm_hip.h; DESIGN.md section 5.7 says what is not known
about judging a window cut from the middle of a read.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N
from .engine import pinned_copy
from .tokenizer import load_tokenizer_from_hyena_model

MODES = ("truncate", "tile")
SPAN_DTYPE = np.dtype([("read", "<i4"), ("src_col", "<i4"), ("n_copy", "<i4"), ("flags", "<i4")])     # struct clm_longread_span
_TOKENIZER = "hyenadna-small-32k-seqlen"


class LongReadError(RuntimeError):
    pass


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


@dataclass(frozen=True)
class Options:
    """How reads longer than the window are treated, validated (`ValueError`).  `mode` "truncate" (the reference's: only the first
    window is seen) or "tile"; `window` in bases (None: what the tokenizer's `max_len_single_sentence` of 32,769 tokens leaves
    beside [SEP]: 32,768); `overlap` of consecutive windows, 0 ... window / 2; `max_bases` >= window, the bases of a read that are
    looked at."""
    mode: str = "tile"
    window: int | None = None
    overlap: int = 4096
    max_bases: int = 262144

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {self.mode!r}")
        for name in ("overlap", "max_bases") + (("window",) if self.window is not None else ()):
            if not _is_int(getattr(self, name)):
                raise ValueError(f"{name} must be an integer, got {getattr(self, name)!r}")
        wb = self.window_bases
        if wb < 1:
            raise ValueError(f"window must be >= 1, got {wb}")
        if not 0 <= 2 * self.overlap <= wb:
            raise ValueError(f"0 <= overlap <= window / 2, got overlap {self.overlap}, window {wb}")
        if self.max_bases < wb:
            raise ValueError(f"max_bases >= window, got max_bases {self.max_bases}, window {wb}")

    @property
    def window_bases(self) -> int:
        if self.window is not None:
            return int(self.window)
        return load_tokenizer_from_hyena_model(_TOKENIZER).max_len_single_sentence - 1     # (the truncating path's row: bases + [SEP])

    @property
    def max_tokens(self) -> int:
        """Tokens of the longest row the data path has to deliver: max_bases and [SEP]."""
        return int(self.max_bases) + 1


def row_lengths(ids) -> np.ndarray:
    """Token counts int32 [B] of a left-padded uint8 batch [B, L] in host memory (`clm_longread_lengths`: a search per row).  Raises
    ValueError for a row of pads only or one that is not pads followed by tokens."""
    if isinstance(ids, torch.Tensor):
        ids = ids.numpy()
    if ids.ndim != 2 or ids.dtype != np.uint8 or ids.strides[1] != 1 or ids.strides[0] < ids.shape[1] or 0 in ids.shape:
        raise ValueError("ids must be a non-empty uint8 [B, L] array with unit column stride")
    out = np.zeros(ids.shape[0], dtype=np.int32)
    lib = N.load()
    if lib.clm_longread_lengths(C.c_void_p(ids.ctypes.data), int(ids.strides[0]), int(ids.shape[0]), int(ids.shape[1]),
                                C.c_void_p(out.ctypes.data)) != 0:
        raise ValueError(lib.clm_longread_last_error(None).decode())
    return out


@dataclass
class Plan:
    """The rows of one batch's forwards (host arrays).  `spans` SPAN_DTYPE [B + n_extra]: the B head rows (`L_out` wide), then the
    extra windows (`C` wide) in read order, then window order; `starts` int32 [B + n_extra] their first base; `first` int32 [B + 1]:
    read r's extra windows are extra rows first[r] ... first[r + 1] - 1; `n_bases` int32 [B] the bases looked at (after the cap)."""
    B: int
    L: int
    L_out: int
    C: int
    first: np.ndarray
    spans: np.ndarray
    starts: np.ndarray
    n_bases: np.ndarray

    @property
    def n_extra(self) -> int:
        return int(self.first[-1])

    @property
    def n_windows(self) -> np.ndarray:
        return 1 + np.diff(self.first)

    def windows_of(self, r: int) -> list[tuple[int, int]]:
        """(row in the [B + n_extra] arrays, first base) of read r's windows, in window order."""
        rows = [r] + list(range(self.B + int(self.first[r]), self.B + int(self.first[r + 1])))
        return [(i, int(self.starts[i])) for i in rows]


def build_plan(lengths, L: int, options: Options | None = None) -> Plan:
    """The plan of a batch whose rows hold `lengths` tokens of `L` (`clm_longread_plan`; host only, needs no GPU)."""
    opt = options if options is not None else Options()
    n_tok = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
    if n_tok.ndim != 1 or n_tok.size < 1:
        raise ValueError("lengths must be a non-empty 1-D array")
    B, wb = int(n_tok.size), opt.window_bases
    lib = N.load()
    L_out, n_spans = C.c_int(0), C.c_int(0)
    first = np.zeros(B + 1, dtype=np.int32)
    args = (C.c_void_p(n_tok.ctypes.data), B, int(L), wb, int(opt.overlap), int(opt.max_bases), C.byref(L_out), C.c_void_p(first.ctypes.data))
    if lib.clm_longread_plan(*args, None, None, 0, C.byref(n_spans)) != 0:
        raise ValueError(lib.clm_longread_last_error(None).decode())
    spans = np.zeros(n_spans.value, dtype=SPAN_DTYPE)
    starts = np.zeros(n_spans.value, dtype=np.int32)
    if lib.clm_longread_plan(*args, C.c_void_p(spans.ctypes.data), C.c_void_p(starts.ctypes.data), n_spans.value, C.byref(n_spans)) != 0:
        raise ValueError(lib.clm_longread_last_error(None).decode())
    return Plan(B, int(L), L_out.value, wb + 1, first, spans, starts, np.minimum(n_tok - 1, opt.max_bases).astype(np.int32))


def needs_windows(lengths, L: int, options: Options) -> bool:
    """Whether `tiled_forward` builds rows for this batch (a read beyond the window, or columns beyond window + 1) or forwards it as
    it is.  The data paths ask before the batch crosses PCIe: only a batch that is rebuilt needs rows the window kernel can read
    (a stride that is a multiple of 16); any other crosses as one contiguous copy, as on the truncating path."""
    c = options.window_bases + 1
    return int(L) > c or int(np.max(lengths)) > c


@dataclass
class TiledLogits:
    """One batch through `tiled_forward`: device tensors, complete when the stream they were queued on reaches them.  `logits` fp32
    [B, 2] the reads' (the chosen windows', bit for bit); `window_logits` fp32 [B + n_extra, 2] (head rows, then extra rows, in the
    plan's order); `chosen` int32 [B]; `gap` fp32 [B + n_extra]; `nonfinite` int32 [B].  For a batch without a long read nothing is
    reduced: `window_logits` is `logits`, the forward's own tensor, and `chosen`, `gap`, `nonfinite` are None."""
    plan: Plan
    logits: torch.Tensor
    window_logits: torch.Tensor
    chosen: torch.Tensor | None = None
    gap: torch.Tensor | None = None
    nonfinite: torch.Tensor | None = None

    def tensors(self) -> dict[str, torch.Tensor]:
        return {k: getattr(self, k) for k in ("logits", "window_logits", "chosen", "gap", "nonfinite") if getattr(self, k) is not None}

    def to_host(self, non_blocking: bool = True) -> "TiledLogits":
        """`engine.pinned_copy` of the tensors."""
        return TiledLogits(self.plan, **pinned_copy(self.tensors(), non_blocking))


class LongReads:
    """One `clm_longread_handle` on `device`: the two kernels on torch's current stream."""

    def __init__(self, device: torch.device | str | int | None = None):
        self._lib = N.load()
        self._h = None
        device = torch.device("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))
        if device.type != "cuda":
            raise LongReadError("the windows are built on an MI355X (torch device type 'cuda' on ROCm) only; there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        if self._lib.clm_longread_create(self.device.index, C.byref(h)) != 0:
            raise LongReadError(self._lib.clm_longread_last_error(None).decode())
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.clm_longread_last_error(self._h).decode()
            raise (ValueError if rc == N.E_INVALID else LongReadError)(msg)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def rows(self, ids: torch.Tensor, spans: torch.Tensor, s0: int, rows: int, out: torch.Tensor, width: int) -> None:
        """Spans s0 ... s0 + rows - 1 of `spans` (int32 [n_spans, 4] on the device) as the first `rows` rows of `out` (uint8
        [>= rows, stride]), `width` bytes each, from the batch `ids` (uint8 [B, L], row stride a multiple of 16)."""
        self._check(self._lib.clm_longread_rows(self._h, C.c_void_p(ids.data_ptr()), int(ids.stride(0)), int(ids.shape[0]),
                                                int(ids.shape[1]), C.c_void_p(spans.data_ptr()), int(spans.shape[0]), int(s0), int(rows),
                                                C.c_void_p(out.data_ptr()), int(out.stride(0)), int(width), self._stream()))

    def reduce(self, logits: torch.Tensor, first: torch.Tensor, B: int, logits_out: torch.Tensor, chosen: torch.Tensor,
               gap: torch.Tensor, nonfinite: torch.Tensor) -> None:
        self._check(self._lib.clm_longread_reduce(self._h, C.c_void_p(logits.data_ptr()), C.c_void_p(first.data_ptr()), int(B),
                                                  C.c_void_p(logits_out.data_ptr()), C.c_void_p(chosen.data_ptr()),
                                                  C.c_void_p(gap.data_ptr()), C.c_void_p(nonfinite.data_ptr()), self._stream()))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.clm_longread_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_handles: dict = {}


def _handle(device: torch.device) -> LongReads:
    if device not in _handles:
        _handles[device] = LongReads(device)
    return _handles[device]


def _round16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


def _forward(net, rows: torch.Tensor) -> torch.Tensor:
    logits = net(rows, None)
    if logits.dtype != torch.float32 or tuple(logits.shape) != (rows.shape[0], 2) or not logits.is_contiguous():
        raise LongReadError(f"the net returned {logits.dtype} {tuple(logits.shape)}, expected contiguous fp32 {(rows.shape[0], 2)}")
    return logits


def tiled_forward(net_or_module, ids: torch.Tensor, *, options: Options | None = None, batch_size: int = 256,
                  lengths=None) -> TiledLogits:
    """The batch `ids` (uint8 [B, L] on the device, padded on the LEFT with [PAD], untruncated) under `net_or_module` -- a net
    (`forward(input_ids, second=None) -> contiguous fp32 logits [rows, 2]`) or a `ClassificationLit` around one -- with every read
    longer than `options.window` cut into overlapping windows.  The head batch goes through the forward whole, as it does today; the
    extra windows follow in chunks of at most `batch_size` rows.  `lengths` (int32 [B], host) are the rows' token counts as the data
    path knows them (`row_lengths` on the host batch); without them the batch is copied back to find them, which waits.  When no
    read is longer than the window and L <= window + 1 no kernel of this module is launched: the batch is forwarded as it is and
    `logits` is the forward's own tensor.  Runs on torch's current stream of the batch's device; does not wait."""
    opt = options if options is not None else Options()
    if opt.mode != "tile":
        raise ValueError("tiled_forward runs options of mode 'tile'")
    if not _is_int(batch_size) or not 1 <= batch_size <= 65535:
        raise ValueError(f"batch_size must be 1 ... 65535, got {batch_size!r}")
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.dtype != torch.uint8 or not ids.is_cuda or 0 in ids.shape \
            or ids.stride(1) != 1:
        raise ValueError("ids must be a non-empty uint8 [B, L] tensor on the device with unit column stride")
    B, L = int(ids.shape[0]), int(ids.shape[1])
    if lengths is None:
        lengths = row_lengths(ids.cpu().numpy())
    plan = build_plan(lengths, L, opt)
    if plan.n_extra == 0 and L <= plan.C:
        logits = _forward(net_or_module, ids)
        return TiledLogits(plan, logits, logits)
    lr = _handle(torch.device("cuda", ids.device.index))
    device, n_extra, n_rows = lr.device, plan.n_extra, B + plan.n_extra
    with torch.inference_mode():
        if ids.data_ptr() % 16 or ids.stride(0) % 16:                # the rows kernel's aligned loads (see the header)
            src = torch.empty((B, _round16(L)), dtype=torch.uint8, device=device)
            src[:, :L].copy_(ids)
            ids = src[:, :L]
        # the plan crosses PCIe once, from page-locked memory (torch's caching host allocator keeps it until the copy is done)
        spans = torch.from_numpy(plan.spans.view(np.int32).reshape(n_rows, 4)).pin_memory().to(device, non_blocking=True)
        first = torch.from_numpy(plan.first).pin_memory().to(device, non_blocking=True)
        window_logits = torch.empty((n_rows, 2), dtype=torch.float32, device=device)
        head = torch.empty((B, _round16(plan.L_out)), dtype=torch.uint8, device=device)
        for r0 in range(0, B, 65535):
            lr.rows(ids, spans, r0, min(65535, B - r0), head[r0:], plan.L_out)
        window_logits[:B].copy_(_forward(net_or_module, head[:, :plan.L_out]))
        if n_extra:
            buf = torch.empty((min(batch_size, n_extra), _round16(plan.C)), dtype=torch.uint8, device=device)   # stream-ordered reuse
            for e0 in range(0, n_extra, batch_size):
                rows = min(batch_size, n_extra - e0)
                lr.rows(ids, spans, B + e0, rows, buf, plan.C)
                window_logits[B + e0: B + e0 + rows].copy_(_forward(net_or_module, buf[:rows, :plan.C]))
        out = TiledLogits(plan, torch.empty((B, 2), dtype=torch.float32, device=device), window_logits,
                          torch.empty((B,), dtype=torch.int32, device=device), torch.empty((n_rows,), dtype=torch.float32, device=device),
                          torch.empty((B,), dtype=torch.int32, device=device))
        lr.reduce(window_logits, first, B, out.logits, out.chosen, out.gap, out.nonfinite)
    return out
