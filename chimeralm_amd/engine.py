"""`Engine`: thin Python owner of one `clm_handle` (one per GPU).  Torch is used only for device memory
and the current HIP stream; all arithmetic happens behind the C ABI (include/chimeralm_hip.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N

_TORCH_DT = {torch.float32: N.DT_F32, torch.float64: N.DT_F64, torch.bfloat16: N.DT_BF16, torch.float16: N.DT_F16}
IDS_DT = {torch.int64: N.DT_I64, torch.int32: N.DT_I32, torch.uint8: N.DT_U8}


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"chimeralm_hip error {code}: {msg}")
        self.code = code


def pinned_copy(tensors: dict[str, torch.Tensor], non_blocking: bool = True) -> dict[str, torch.Tensor]:
    """Copies of `tensors` in page-locked host memory, queued on the current stream: wait for an event behind them before reading.
    (Host tensors -- the CPU rehearsals of the tests -- are copied to ordinary memory.)"""
    host = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=v.is_cuda) for k, v in tensors.items()}
    for k, v in tensors.items():
        host[k].copy_(v, non_blocking=non_blocking)
    return host


@dataclass(frozen=True)
class AttentionRequest:
    """What a forward should also leave on the device (`clm_forward_attn`): per read the summary record and the `top_k` (1 ... 32)
    largest-weight bases -- `top_k=None`: not wanted -- and / or the softmax weights of every position."""
    top_k: int | None = 10
    weights: bool = False

    def __post_init__(self):
        if self.top_k is None and not self.weights:
            raise ValueError("an attention request asks for peaks (top_k), weights, or both")
        if self.top_k is not None and not 1 <= int(self.top_k) <= N.ATTN_MAX_TOP_K:
            raise ValueError(f"top_k must be 1 ... {N.ATTN_MAX_TOP_K}")


@dataclass
class AttentionOutput:
    """Device tensors of one batch, complete when the forward's stream reaches them (nothing here synchronises).
    `summary` int32 [B, 8] is the batch's `clm_attn_summary` records (`fields()` names the columns), `peak_pos` int32 [B, top_k]
    0-based positions among a read's bases (token index = position + n_pad; -1 beyond n_peaks), `peak_weight` fp32 [B, top_k],
    `weights` fp32 [B, L] the softmax over all positions, [PAD] and [SEP] included.  Parts not asked for are None."""
    top_k: int | None
    summary: torch.Tensor | None = None
    peak_pos: torch.Tensor | None = None
    peak_weight: torch.Tensor | None = None
    weights: torch.Tensor | None = None

    def tensors(self) -> dict[str, torch.Tensor]:
        return {k: v for k, v in (("summary", self.summary), ("peak_pos", self.peak_pos), ("peak_weight", self.peak_weight),
                                  ("weights", self.weights)) if v is not None}

    def to_host(self, non_blocking: bool = True) -> "AttentionOutput":
        """`pinned_copy` of the parts that are there."""
        return AttentionOutput(self.top_k, **pinned_copy(self.tensors(), non_blocking))

    def fields(self) -> dict[str, torch.Tensor]:
        """The summary's columns by name (views): n_pad, n_bases, has_sep, n_peaks int32; pad_weight, sep_weight, base_weight fp32."""
        if self.summary is None:
            return {}
        f = self.summary.view(torch.float32)
        out = {n: self.summary[:, i] for i, n in enumerate(("n_pad", "n_bases", "has_sep", "n_peaks"))}
        out.update({n: f[:, 4 + i] for i, n in enumerate(("pad_weight", "sep_weight", "base_weight"))})
        return out


TRAJ_FIELDS = ("n_pad", "n_bases", "has_sep", "n_points", "first_k", "label", "onset_k", "jump_k", "n_nonfinite", "reserved",
               "jump_dgap", "final_gap")             # clm_traj_summary: ten int32, then two fp32


def check_trajectory_stride(stride: int) -> int:
    stride = int(stride)
    if not N.TRAJ_STRIDE_UNIT <= stride <= N.TRAJ_STRIDE_MAX or stride % N.TRAJ_STRIDE_UNIT:
        raise ValueError(f"a trajectory's stride must be a multiple of {N.TRAJ_STRIDE_UNIT} in {N.TRAJ_STRIDE_UNIT} ... {N.TRAJ_STRIDE_MAX}")
    return stride


def bases_seen(n_points: int, stride: int, length: int, n_pad, n_bases) -> np.ndarray:
    """int32 [B, K]: the bases of each read that lie inside point k, clamp(n_k - n_pad, 0, n_bases) with n_k = min((k + 1) S, L)."""
    n_k = np.minimum((np.arange(n_points, dtype=np.int64) + 1) * int(stride), int(length))
    n_pad, n_bases = np.asarray(n_pad, np.int64)[:, None], np.asarray(n_bases, np.int64)[:, None]
    return np.clip(n_k[None, :] - n_pad, 0, n_bases).astype(np.int32)


@dataclass(frozen=True)
class TrajectoryRequest:
    """What a forward should also leave on the device (`clm_forward_traj`): the logits the model would give if a row ended after
    (k + 1) * `stride` of its tokens, for every such point (the last point is the row itself), and per read the summary record."""
    stride: int = 128
    summary: bool = True

    def __post_init__(self):
        check_trajectory_stride(self.stride)


@dataclass
class TrajectoryOutput:
    """Device tensors of one batch, complete when the forward's stream reaches them (nothing here synchronises).  `logits` fp32
    [B, K, 2], K = ceil(length / stride) points per row of `length` tokens; `summary` int32 [B, 12], the batch's `clm_traj_summary`
    records (`fields()` names the columns), or None."""
    stride: int
    length: int
    logits: torch.Tensor
    summary: torch.Tensor | None = None

    def tensors(self) -> dict[str, torch.Tensor]:
        return {k: v for k, v in (("logits", self.logits), ("summary", self.summary)) if v is not None}

    def to_host(self, non_blocking: bool = True) -> "TrajectoryOutput":
        """`pinned_copy` of the parts that are there."""
        return TrajectoryOutput(self.stride, self.length, **pinned_copy(self.tensors(), non_blocking))

    def fields(self) -> dict[str, torch.Tensor]:
        """The summary's columns by name (views): ten int32, then jump_dgap and final_gap fp32."""
        if self.summary is None:
            return {}
        f = self.summary.view(torch.float32)
        return {n: (self.summary if i < 10 else f)[:, i] for i, n in enumerate(TRAJ_FIELDS)}

    def bases_seen(self) -> np.ndarray:
        """int32 [B, K] from HOST tensors with a summary: the bases of each read inside each point."""
        f = self.fields()
        return bases_seen(self.logits.shape[1], self.stride, self.length, f["n_pad"].numpy(), f["n_bases"].numpy())


def trajectory_out(req: TrajectoryRequest | None, B: int, L: int, device: torch.device):
    """Device tensors for a trajectory request (torch's allocator, like the logits) and a reference to the `clm_traj_out` that points
    at them, as the C calls take it (`clm_forward_traj`, `clm_mamba_forward_traj`); (None, None) without a request."""
    if req is None:
        return None, None
    B, L = int(B), int(L)
    K = (L + req.stride - 1) // req.stride
    t = TrajectoryOutput(int(req.stride), L, torch.empty((B, K, 2), dtype=torch.float32, device=device),
                         torch.empty((B, len(TRAJ_FIELDS)), dtype=torch.int32, device=device) if req.summary else None)
    c = N.ClmTrajOut()
    c.struct_size, c.stride, c.logits, c.point_stride = C.sizeof(N.ClmTrajOut), t.stride, t.logits.data_ptr(), K
    c.summary = t.summary.data_ptr() if t.summary is not None else None
    return t, C.byref(c)


class _DevicePtr:
    """fp32 device memory somebody else owns, as torch sees it through `__cuda_array_interface__`."""

    def __init__(self, ptr: int, shape: tuple[int, ...]):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}


def _device_view(ptr: int, shape: tuple[int, ...], device: torch.device) -> torch.Tensor:
    return torch.as_tensor(_DevicePtr(ptr, shape), device=device)


class Engine:
    """One MI355X inference engine instance bound to `device` (e.g. "cuda:0")."""

    def __init__(self, device: torch.device | str | int = "cuda:0", precision: str = "fp32", chunk_reads: int = 256):
        self._lib = N.load()
        self._h = N._H()
        device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if device.type != "cuda":
            raise EngineError(N.E_UNSUPPORTED, "the engine runs on an MI355X (torch device type 'cuda' on ROCm) only; "
                                               "there is no CPU path")
        if precision not in N.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(N.PRECISIONS)}")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        self.precision = precision
        cfg = N.ClmConfig()
        self._lib.clm_default_config(C.byref(cfg))
        cfg.precision = N.PRECISIONS[precision]
        cfg.chunk_reads = int(chunk_reads)
        self.cfg = cfg
        rc = self._lib.clm_create(C.byref(cfg), self.device.index, C.byref(self._h))
        if rc:
            raise EngineError(rc, (self._lib.clm_last_error(None) or b"").decode())
        self.finalized = False

    # ------------------------------------------------------------------ helpers
    def _check(self, rc: int):
        if rc:
            raise EngineError(rc, (self._lib.clm_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.clm_destroy(self._h)
            self._h = N._H()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    # ------------------------------------------------------------------ weights
    def load_weight(self, key: str, tensor: torch.Tensor):
        t = tensor.detach()
        if t.dtype not in _TORCH_DT:
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        self._check(self._lib.clm_load_weight(self._h, key.encode(), C.c_void_p(t.data_ptr()), _TORCH_DT[t.dtype],
                                              shape, t.dim()))
        self.finalized = False

    def load_state_dict(self, state_dict: dict[str, torch.Tensor]):
        """Load every `net.backbone.*` / `net.head.*` entry of a reference checkpoint and finalize."""
        for k, v in state_dict.items():
            kk = k[4:] if k.startswith("net.") else k
            if kk.startswith("backbone.") or kk.startswith("head."):
                self.load_weight(k, v)
        self.finalize()

    def finalize(self):
        self._check(self._lib.clm_finalize(self._h))
        self.finalized = True

    def reserve(self, batch: int, length: int):
        self._check(self._lib.clm_reserve(self._h, int(batch), int(length)))

    # ------------------------------------------------------------------ forward
    def _attn_out(self, req: AttentionRequest | None, B: int, L: int):
        """Device tensors for a request (torch's allocator, like the logits) and a reference to the `clm_attn_out` that points at
        them, as the C call takes it; (None, None) without a request."""
        if req is None:
            return None, None
        B, L = int(B), int(L)
        a = AttentionOutput(None if req.top_k is None else int(req.top_k))
        c = N.ClmAttnOut()
        c.struct_size = C.sizeof(N.ClmAttnOut)
        if req.weights:
            a.weights = torch.empty((B, L), dtype=torch.float32, device=self.device)
            c.weights, c.weights_row_stride = a.weights.data_ptr(), L
        if a.top_k is not None:
            a.summary = torch.empty((B, 8), dtype=torch.int32, device=self.device)
            a.peak_pos = torch.empty((B, a.top_k), dtype=torch.int32, device=self.device)
            a.peak_weight = torch.empty((B, a.top_k), dtype=torch.float32, device=self.device)
            c.top_k, c.summary, c.peak_pos, c.peak_weight = a.top_k, a.summary.data_ptr(), a.peak_pos.data_ptr(), a.peak_weight.data_ptr()
        return a, C.byref(c)

    def _traj_out(self, req: TrajectoryRequest | None, B: int, L: int):
        """The same for a trajectory request and its `clm_traj_out`."""
        return trajectory_out(req, B, L, self.device)

    @staticmethod
    def _result(out, att, trj):
        """`out`, `(out, att)`, `(out, trj)` or `(out, att, trj)`: the logits alone, or a tuple with what was asked for."""
        return out if att is None and trj is None else tuple(x for x in (out, att, trj) if x is not None)

    def forward(self, input_ids: torch.Tensor, out: torch.Tensor | None = None, attention: AttentionRequest | None = None,
                trajectory: TrajectoryRequest | None = None):
        """input_ids [B, L] (int64 / int32 / uint8) on this engine's device -> logits fp32 [B, 2]; with an `attention` request
        -> (logits, AttentionOutput), with a `trajectory` request -> (logits, TrajectoryOutput), with both -> (logits,
        AttentionOutput, TrajectoryOutput), written by the same call for every chunk of the batch (`clm_forward_traj`).
        Asynchronous on torch's current stream."""
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [batch, length]")
        if input_ids.device != self.device:
            raise EngineError(N.E_INVALID, f"input_ids is on {input_ids.device}, engine on {self.device}; "
                                           "no CPU execution path exists")
        if input_ids.dtype not in IDS_DT:
            raise ValueError("input_ids dtype must be int64, int32 or uint8")
        if input_ids.stride(1) != 1:
            input_ids = input_ids.contiguous()
        B, L = input_ids.shape
        if out is None:
            out = torch.empty((B, self.cfg.n_classes), dtype=torch.float32, device=self.device)
        (att, c), (trj, ct) = self._attn_out(attention, B, L), self._traj_out(trajectory, B, L)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_forward_traj(self._h, C.c_void_p(input_ids.data_ptr()), IDS_DT[input_ids.dtype], input_ids.stride(0), B, L,
                                               C.c_void_p(out.data_ptr()), c, ct, C.c_void_p(stream)))
        return self._result(out, att, trj)

    __call__ = forward

    # ------------------------------------------------------------------ host batches (pinned slots of the BAM feeder)
    def stage_host_ids(self, host_ptr: int, ids_dtype: int, row_stride: int, batch: int, length: int) -> int:
        """Enqueue the H2D copy of a host batch on the engine's own copy stream (overlaps the running forward);
        returns the staging-buffer index to pass to `forward_staged` / `stage_wait`."""
        k = C.c_int(-1)
        self._check(self._lib.clm_stage_ids(self._h, C.c_void_p(host_ptr), int(ids_dtype), int(row_stride), int(batch),
                                            int(length), C.byref(k)))
        return k.value

    def forward_staged(self, staged: int, batch: int, out: torch.Tensor | None = None,
                       attention: AttentionRequest | None = None, length: int | None = None,
                       trajectory: TrajectoryRequest | None = None):
        """The forward of a staged batch of `batch` reads; with an `attention` and / or `trajectory` request (then `length`, the
        batch's tokens per read, is needed to size the outputs) the same tuples as `forward`."""
        if out is None:
            out = torch.empty((batch, self.cfg.n_classes), dtype=torch.float32, device=self.device)
        if length is None and (attention is not None or trajectory is not None):
            raise ValueError("forward_staged with an attention or trajectory request needs the batch's `length`")
        (att, c), (trj, ct) = self._attn_out(attention, batch, length), self._traj_out(trajectory, batch, length)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_forward_staged_traj(self._h, int(staged), C.c_void_p(out.data_ptr()), c, ct, C.c_void_p(stream)))
        return self._result(out, att, trj)

    def check(self):
        """Wait for the current stream and raise for errors only the device can see (token ids outside the embedding table:
        the reference raises IndexError there)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_check(self._h, C.c_void_p(stream)))

    # ------------------------------------------------------------------ 16-bit mode vs the reference's arithmetic
    def selfcheck(self, input_ids: torch.Tensor) -> tuple[float, int]:
        """Run `input_ids` through this engine's mode AND through the exact-fp32 kernels of the same handle; returns
        (max |logit difference|, number of reads whose label differs).  Synchronises the current stream (`clm_selfcheck`)."""
        if input_ids.dim() != 2 or input_ids.device != self.device or input_ids.dtype not in IDS_DT:
            raise ValueError("selfcheck wants input_ids [batch, length] (int64 / int32 / uint8) on the engine's device")
        if input_ids.stride(1) != 1:
            input_ids = input_ids.contiguous()
        B, L = input_ids.shape
        diff, differ = C.c_float(0.0), C.c_int(0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_selfcheck(self._h, C.c_void_p(input_ids.data_ptr()), IDS_DT[input_ids.dtype],
                                            input_ids.stride(0), B, L, C.c_void_p(stream), C.byref(diff), C.byref(differ)))
        return float(diff.value), int(differ.value)

    def set_fallback(self, level: int | bool = 1):
        """`clm_set_fallback`: 0 = the engine's own mode; 1 = every later forward runs in the next arithmetic inside the 1e-3 gate
        (a 16-bit engine: fp16x3, fp32-class logits at about twice the exact rate; an fp16x3 engine: exact fp32); 2 = exact fp32."""
        self._check(self._lib.clm_set_fallback(self._h, int(level)))

    def set_f16c_min_len(self, min_len: int):
        """fp16c: reads shorter than `min_len` tokens run in the fp16x3 kernels (`clm_set_short_read_len`)."""
        self._check(self._lib.clm_set_short_read_len(self._h, int(min_len)))

    def set_mlp_compensation(self, on: bool = True):
        """fp16c: fc1 / fc2 on hi + lo weights too (`clm_set_mlp_compensation`; ~10 % slower, for weights whose MLP rounding shows)."""
        self._check(self._lib.clm_set_mlp_compensation(self._h, int(on)))

    def effective_precision(self, length: int) -> str:
        code = self._lib.clm_effective_precision(self._h, int(length))
        if code < 0:
            raise EngineError(code, "clm_effective_precision")
        return N.PREC_NAMES[code]

    def stage_wait(self, staged: int):
        self._check(self._lib.clm_stage_wait(self._h, int(staged)))

    # ------------------------------------------------------------------ the head fine-tune (headtrain.py)
    def chunk_reads_for(self, length: int) -> int:
        """Reads of `length` tokens this engine runs as ONE chunk (`clm_chunk_reads`): the most whose rows `rows()` hands out."""
        n = int(self._lib.clm_chunk_reads(self._h, int(length)))
        if n < 1:
            raise EngineError(n, "clm_chunk_reads: the engine is not finalized, or length < 1")
        return n

    def rows_generation(self) -> int:
        """Moves whenever the engine may have rewritten the rows `rows()` returned (every forward, every weight load)."""
        return int(self._lib.clm_rows_generation(self._h))

    def rows(self) -> torch.Tensor:
        """The final residual rows fp32 [B, L, 256] (before ln_f) the last forward left: a VIEW of the engine's workspace, not a copy
        -- valid until `rows_generation()` moves.  Raises unless that forward ran one chunk (B <= chunk_reads) on the exact-fp32 or
        fp16x3 kernels (`clm_rows`)."""
        ptr, B, L = C.c_void_p(), C.c_int(), C.c_int()
        self._check(self._lib.clm_rows(self._h, C.byref(ptr), C.byref(B), C.byref(L)))
        return _device_view(ptr.value, (B.value, L.value, 256), self.device)

    def _f32(self, name: str, t: torch.Tensor | None, numel: int | None = None) -> C.c_void_p:
        if t is None:
            return C.c_void_p(None)
        if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 tensor on {self.device}")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{name} must hold {numel} values, got {tuple(t.shape)}")
        return C.c_void_p(t.data_ptr()) if t.numel() else C.c_void_p(None)

    @staticmethod
    def _rows_shape(rows: torch.Tensor | None) -> tuple[int, int]:
        if rows is None:
            return 0, 0
        if rows.dim() != 3 or rows.shape[2] != 256:
            raise ValueError("rows must be [batch, length, 256]")
        return int(rows.shape[0]), int(rows.shape[1])

    def pool_forward(self, rows, w1, b1, w2, b2):
        """Attention pooling of `rows` [B, L, 256] under the given weights (attention.0 weight [256, 256] and bias [256], attention.2
        weight [256] values and bias [1]; ln_f is the engine's) -> (scores [B, L], stats [B, 2] = max and sum, pooled [B, 256]).
        Asynchronous on torch's current stream (`clm_pool_forward`)."""
        B, L = self._rows_shape(rows)
        args = [self._f32("rows", rows), B, L, self._f32("w1", w1, 65536), self._f32("b1", b1, 256), self._f32("w2", w2, 256),
                self._f32("b2", b2, 1)]
        scores = torch.empty((B, L), dtype=torch.float32, device=self.device)
        stats = torch.empty((B, 2), dtype=torch.float32, device=self.device)
        pooled = torch.empty((B, 256), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_pool_forward(self._h, *args, self._f32("scores", scores), self._f32("stats", stats),
                                               self._f32("pooled", pooled), C.c_void_p(stream)))
        return scores, stats, pooled

    def pool_backward(self, rows, w1, b1, w2, scores, stats, pooled, dpooled, out=None, beta: float = 0.0):
        """Gradients of the pooling's four tensors given dloss/dpooled [B, 256] and what `pool_forward` returned for the same rows and
        weights -> (d_w1 [256, 256], d_b1 [256], d_w2 [256], d_b2 [1]); with `out` (such a tuple) and beta = 1 they are added to it.
        Exact fp32, bitwise repeatable (`clm_pool_backward`)."""
        B, L = self._rows_shape(rows)
        if out is None:
            if beta != 0.0:
                raise ValueError("beta = 1 accumulates into `out`")
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in ((256, 256), (256,), (256,), (1,)))
        args = [self._f32("rows", rows), B, L, self._f32("w1", w1, 65536), self._f32("b1", b1, 256), self._f32("w2", w2, 256),
                self._f32("scores", scores, B * L), self._f32("stats", stats, B * 2), self._f32("pooled", pooled, B * 256),
                self._f32("dpooled", dpooled, B * 256), self._f32("d_w1", out[0], 65536), self._f32("d_b1", out[1], 256),
                self._f32("d_w2", out[2], 256), self._f32("d_b2", out[3], 1)]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.clm_pool_backward(self._h, *args, C.c_float(beta), C.c_void_p(stream)))
        return out

    # ------------------------------------------------------------------ taps
    def debug_stop_after(self, layer: int = -1, stage: int = -1):
        self._check(self._lib.clm_debug_stop_after(self._h, layer, stage))

    def debug_fetch(self, name: str, shape, dtype=np.float32) -> np.ndarray:
        arr = np.empty(shape, dtype=dtype)
        self._check(self._lib.clm_debug_fetch(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def profile_enable(self, on: bool = True):
        self._check(self._lib.clm_profile_enable(self._h, int(on)))

    def profile_read(self, reset: bool = True) -> dict[str, tuple[float, int]]:
        ms = (C.c_double * N.N_STAGES)()
        n = (C.c_int64 * N.N_STAGES)()
        self._check(self._lib.clm_profile_read(self._h, ms, n, int(reset)))
        return {N.STAGES[i]: (ms[i], n[i]) for i in range(N.N_STAGES)}
