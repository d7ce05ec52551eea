"""Length-bucketed predict: a read's row -- and so its logits -- depends on the read alone, behind the `clm_bucket_*` C ABI
(csrc/bucket_plan.cpp, csrc/bucket.hip), for any net.

The reference pads a batch on the left to its longest read (/root/reference/chimeralm/data/tokenizer.py:152-159) and masks nothing:
the same read gets other logits, and possibly another label, next to other reads, and a ragged file pays for the pads.  Here every
read is padded to a canonical length that is a function of its own token count, and reads of one canonical length are forwarded
together.  `regroup` sits between the loops' staged device batches and `predict_step`: the planner says where each read's bytes go in
a pool of per-class slabs, one small kernel moves them on torch's current stream, and a class that is full (or, at the end of the
input, holds anything) is yielded as an ordinary batch.  The nets do not change; the left pads differ from the reference's, so this
mode is not reference parity.  The definitions are in include/chimeralm_hip.h; DESIGN.md section 5.8 says what is invariant for
which net.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N

log = logging.getLogger(__name__)

MODES = ("file", "bucket")
SPAN_DTYPE = np.dtype([("src_row", "<i4"), ("src_col", "<i4"), ("n_copy", "<i4"), ("dst_width", "<i4"),
                       ("dst_offset", "<i8")])                                                        # struct clm_bucket_span
STEP_DTYPE = np.dtype([("kind", "<i4"), ("first", "<i4"), ("count", "<i4"), ("length", "<i4"), ("offset", "<i8"),
                       ("stride", "<i8")])                                                            # struct clm_bucket_step


class BucketError(RuntimeError):
    pass


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


@dataclass(frozen=True)
class Options:
    """How predict batches are formed, validated (`ValueError`).  `mode` "file" (the reference's: batches in file order, padded to
    their longest read) or "bucket"; `steps_log2` 0 ... 5: 2^steps_log2 canonical lengths per octave above 1,024 bases."""
    mode: str = "bucket"
    steps_log2: int = 3

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {self.mode!r}")
        if not _is_int(self.steps_log2) or not 0 <= self.steps_log2 <= 5:
            raise ValueError(f"steps_log2 must be an integer 0 ... 5, got {self.steps_log2!r}")


def canonical_length(n: int, options: Options | None = None) -> int:
    """Tokens of the row a read of `n` tokens (its bases and [SEP]) is forwarded in: Lc(n) of the header."""
    opt = options if options is not None else Options()
    lib = N.load()
    lc = lib.clm_bucket_length(int(n), int(opt.steps_log2)) if _is_int(n) else -1
    if lc < 0:
        raise ValueError(f"a read has 1 ... {N.BUCKET_MAX_TOKENS} tokens, got {n!r}")
    return lc


def pool_bytes(batch_size: int, options: Options | None = None) -> int:
    """Bytes of the pool with every class present: batch_size rows of round16(Lc) bytes per class."""
    opt = options if options is not None else Options()
    lib = N.load()
    n = lib.clm_bucket_pool_bytes(int(batch_size), int(opt.steps_log2)) if _is_int(batch_size) else -1
    if n < 0:
        raise ValueError(f"batch_size must be 1 ... 65535, got {batch_size!r}")
    return int(n)


class Planner:
    """One `clm_bucket_plan`: host only, needs no GPU.  `push` and `finish` return (steps STEP_DTYPE, spans SPAN_DTYPE, reads int64)
    as copies."""

    def __init__(self, batch_size: int, options: Options | None = None):
        opt = options if options is not None else Options()
        self._lib = N.load()
        self._p = None
        p = C.c_void_p()
        if not _is_int(batch_size) or self._lib.clm_bucket_plan_create(int(batch_size), int(opt.steps_log2), C.byref(p)) != 0:
            raise ValueError(f"batch_size must be 1 ... 65535, got {batch_size!r}")
        self._p, self.batch_size, self.options = p, int(batch_size), opt

    def _steps(self):
        ptr = [C.c_void_p() for _ in range(3)]
        n = [C.c_int() for _ in range(3)]
        if self._lib.clm_bucket_plan_steps(self._p, C.byref(ptr[0]), C.byref(n[0]), C.byref(ptr[1]), C.byref(n[1]), C.byref(ptr[2]),
                                           C.byref(n[2])) != 0:
            raise BucketError("clm_bucket_plan_steps failed")
        out = []
        for p, k, dt in zip(ptr, n, (STEP_DTYPE, SPAN_DTYPE, np.dtype("<i8"))):
            out.append(np.frombuffer(C.string_at(p.value, k.value * dt.itemsize), dtype=dt).copy() if k.value else np.zeros(0, dtype=dt))
        return tuple(out)

    def push(self, lengths, L: int):
        n_tok = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
        if n_tok.ndim != 1 or n_tok.size < 1:
            raise ValueError("lengths must be a non-empty 1-D array")
        if self._lib.clm_bucket_plan_push(self._p, C.c_void_p(n_tok.ctypes.data), int(n_tok.size), int(L)) != 0:
            raise ValueError(self._lib.clm_bucket_plan_last_error(self._p).decode())
        return self._steps()

    def finish(self):
        if self._lib.clm_bucket_plan_finish(self._p) != 0:
            raise BucketError("clm_bucket_plan_finish failed")
        return self._steps()

    def close(self) -> None:
        if getattr(self, "_p", None) is not None:
            self._lib.clm_bucket_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scatter:
    """One `clm_bucket_handle` on `device`: the scatter kernel on torch's current stream."""

    def __init__(self, device: torch.device | str | int | None = None):
        self._lib = N.load()
        self._h = None
        device = torch.device("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))
        if device.type != "cuda":
            raise BucketError("the bucket rows are built on an MI355X (torch device type 'cuda' on ROCm) only; there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        if self._lib.clm_bucket_create(self.device.index, C.byref(h)) != 0:
            raise BucketError(self._lib.clm_bucket_last_error(None).decode())
        self._h = h

    def scatter(self, ids: torch.Tensor, spans: np.ndarray, s0: int, rows: int, pool: torch.Tensor) -> None:
        """Spans s0 ... s0 + rows - 1 of `spans` (SPAN_DTYPE, host) from the batch `ids` (uint8 [B, L] on the device, row stride a
        multiple of 16) into `pool` (uint8, flat, on the device)."""
        if spans.dtype != SPAN_DTYPE or spans.ndim != 1 or not spans.flags.c_contiguous:
            raise ValueError("spans must be a contiguous 1-D SPAN_DTYPE array")
        rc = self._lib.clm_bucket_scatter(self._h, C.c_void_p(ids.data_ptr()), int(ids.stride(0)), int(ids.shape[0]), int(ids.shape[1]),
                                          C.c_void_p(spans.ctypes.data), int(spans.shape[0]), int(s0), int(rows),
                                          C.c_void_p(pool.data_ptr()), int(pool.numel()),
                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            msg = self._lib.clm_bucket_last_error(self._h).decode()
            raise (ValueError if rc == N.E_INVALID else BucketError)(msg)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.clm_bucket_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _round16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


class Regrouper:
    """The state of one bucketed predict run on `device`: the planner, the pool of per-class slabs on the device, and per class the
    host arrays of the `id` rows and labels of the reads its slab holds."""

    def __init__(self, device: torch.device | str | int | None, batch_size: int, options: Options | None = None):
        opt = options if options is not None else Options()
        if opt.mode != "bucket":
            raise ValueError("a Regrouper runs options of mode 'bucket'")
        self.planner = Planner(batch_size, opt)
        self.kernel = Scatter(device)
        self.device, self.batch_size, self.options = self.kernel.device, int(batch_size), opt
        size = pool_bytes(batch_size, opt)
        self.pool = torch.empty((size,), dtype=torch.uint8, device=self.device)
        log.info("bucketed predict: pool of %s bytes on %s (batch size %d, %d canonical lengths per octave)", f"{size:,}", self.device,
                 batch_size, 1 << opt.steps_log2)
        self._host: dict[int, tuple[np.ndarray, np.ndarray]] = {}       # Lc -> (id rows [batch_size, W], labels [batch_size])
        self._slab: dict[int, int] = {}                                # Lc -> the slab's offset in the pool
        self.n_batches = self.n_rows = self.n_tokens = 0               # emitted so far: what the forwards were given

    def _class(self, lc: int, first_offset: int, id_rows: np.ndarray, labels: np.ndarray):
        if lc not in self._host:                                       # the class's first read is row 0 of its slab
            self._slab[lc] = first_offset
            self._host[lc] = (np.zeros((self.batch_size, *id_rows.shape[1:]), dtype=id_rows.dtype),
                              np.zeros(self.batch_size, dtype=labels.dtype))
        return self._host[lc]

    def _emit(self, step) -> dict:
        lc, rows, stride = int(step["length"]), int(step["count"]), int(step["stride"])
        slab = self.pool[int(step["offset"]): int(step["offset"]) + rows * stride].view(rows, stride)
        ids, labels = self._host[lc]
        self.n_batches += 1
        self.n_rows += rows
        self.n_tokens += rows * lc
        return {"input_ids": slab[:, :lc], "id": torch.from_numpy(ids[:rows].copy()), "labels": torch.from_numpy(labels[:rows].copy())}

    def push(self, batch: dict):
        """One staged batch -- `input_ids` uint8 [B, L] on the device, padded on the LEFT, `id` and `labels` on the host, `lengths`
        (int32 [B], host) its rows' token counts as found before the copy; without them the batch is copied back, which waits --
        into the slabs; yields the batches that became full, in the order they did."""
        ids = batch["input_ids"]
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.dtype != torch.uint8 or not ids.is_cuda or 0 in ids.shape \
                or ids.stride(1) != 1:
            raise ValueError("input_ids must be a non-empty uint8 [B, L] tensor on the device with unit column stride")
        B, L = int(ids.shape[0]), int(ids.shape[1])
        lengths = batch.get("lengths")
        if lengths is None:
            from .longread import row_lengths

            lengths = row_lengths(ids.cpu().numpy())
        id_rows = np.asarray(batch["id"])
        labels = np.asarray(batch["labels"])
        if id_rows.shape[0] != B or labels.shape[0] != B:
            raise ValueError(f"the batch has {B} rows, {id_rows.shape[0]} id rows and {labels.shape[0]} labels")
        steps, spans, reads = self.planner.push(lengths, L)
        if ids.data_ptr() % 16 or ids.stride(0) % 16:                 # the scatter kernel's aligned loads (see the header)
            src = torch.empty((B, _round16(L)), dtype=torch.uint8, device=self.device)
            src[:, :L].copy_(ids)
            ids = src[:, :L]
        for step in steps:
            if step["kind"] == N.BUCKET_EMIT:
                yield self._emit(step)
                continue
            s0, n = int(step["first"]), int(step["count"])
            for r0 in range(0, n, 65535):
                self.kernel.scatter(ids, spans, s0 + r0, min(65535, n - r0), self.pool)
            group = spans[s0: s0 + n]
            widths, at = np.unique(group["dst_width"], return_index=True)
            for lc in widths[np.argsort(at)]:                         # the reads' id rows and labels follow them, class by class
                mine = group[group["dst_width"] == lc]
                host_ids, host_labels = self._class(int(lc), int(mine["dst_offset"][0]), id_rows, labels)
                slots = (mine["dst_offset"] - self._slab[int(lc)]) // _round16(int(lc))
                host_ids[slots] = id_rows[mine["src_row"]]
                host_labels[slots] = labels[mine["src_row"]]

    def finish(self):
        """The classes that still hold rows, in ascending canonical length."""
        steps, _spans, _reads = self.planner.finish()
        for step in steps:
            yield self._emit(step)

    def close(self) -> None:
        self.planner.close()
        self.kernel.close()


def regroup(staged_batches, regrouper: Regrouper):
    """The batches of a bucketed run from the loops' staged device batches (see `Regrouper.push`): ordinary batch dicts, `input_ids` a
    [rows, Lc] view of a slab.  A yielded batch is forwarded on torch's current stream before the generator is advanced: the stream
    orders the forward in front of the scatter that refills the slab."""
    for batch in staged_batches:
        yield from regrouper.push(batch)
    yield from regrouper.finish()
