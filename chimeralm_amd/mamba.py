"""Drop-ins for the reference's two Mamba nets (chimeralm/models/components/mamba.py; configs/model/mamba.yaml and mambasp.yaml),
with the forward on MI355X.

`MambaSequenceClassification` (`model: mamba`) and `MambaSequenceClassificationSP` (`model: mambasp`) take the reference's
constructor arguments, have its `state_dict()` keys and shapes (`mamba_layers.3.mamba.A_log`, `mamba_layers.1.out_proj.weight`,
...), its `forward(input_ids, second_arg=None) -> logits [B, 2]` in eval mode (dropout off) and the `number_of_classes` attribute
`ClassificationLit` reads.  The reference builds its layers from `mamba_ssm.Mamba2` (CUDA / Triton only); `Mamba2` here is a
parameter container with the same names, shapes and initialisation.  The arithmetic runs in csrc/mamba.hip behind the
`clm_mamba_*` C ABI; there is no CPU path.  Token ids outside [0, 12) are clamped into the table (the reference's nn.Embedding raises).

`mamba` multiplies its hidden states by the second forward argument (`attention_mask`; `ClassificationLit` passes `input_quals`
there, None on the predict path) and raises for reads longer than `model_max_length`.  `mambasp` ignores the second argument.

Engine knob absent in the reference: `precision` -- "fp16x3" (the default: in_proj, out_proj and the `mamba` front Linear as three
fp16 MFMAs on hi + lo halfs per product) or "fp32" (the exact-fp32 MFMA).  The scan, the norms and the head are fp32 in both.  fp16x3
packs weights x 2^10 as fp16 halfs, which saturates for |w| >= 64 (out_proj counted with norm.weight folded in): such weights run
the exact-fp32 kernels, with a warning and a `precision_report` entry.  An activation beyond fp16's range makes the fp16x3 kernels
return NaN for it; a batch whose fp16x3 logits are not all finite is rerun on the exact-fp32 kernels, logged and recorded.

The running verdict, as for `HyenaDna` (csrc/mamba_verdict.hip): both nets are causal, so with the keyword `trajectory_stride` set
every forward also leaves `last_trajectory`, an `engine.TrajectoryOutput` of DEVICE tensors -- the logits the model would give if a
row ended at each multiple of the stride, and the per-read summary -- from the same call (`clm_mamba_forward_traj`).  After a
non-finite fp16x3 rerun it is the trajectory of the exact-fp32 handle, whose logits were returned.

Training (mambatrain.py, csrc/mamba_train.hip): with the keyword `trainable=True`, in `train()` and with autograd on, the forward runs
the Mamba2 core forward and backward on the engine, the rest in torch, and returns logits with a graph to every parameter; dropout is
then active.  Every other call -- `trainable=False`, `eval()`, `no_grad` -- is the inference forward above, bit for bit.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from functools import partial

import numpy as np
import torch
from torch import nn

from . import _native as N
from ._guard import x3_range_report
from ._reload import reload_signature
from .engine import IDS_DT, TrajectoryRequest, check_trajectory_stride, trajectory_out

HEADDIM, D_CONV, VOCAB, PAD = 64, 4, 12, 4
_LOG = logging.getLogger("chimeralm_amd")


class MambaEngineError(RuntimeError):
    pass


class _Norm(nn.Module):
    def __init__(self, n: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))


class Mamba2(nn.Module):
    """`mamba_ssm.Mamba2`'s parameters under its names, initialised as mamba_ssm does: A uniform in [1, 16] (A_log = log A), dt
    log-uniform in [1e-3, 0.1] (floored at 1e-4) through the inverse softplus into dt_bias, D = 1, norm.weight = 1; in_proj, conv1d
    and out_proj keep torch's default initialisation.  No forward of its own: inference runs the whole net on the MI355X engine,
    training runs this layer through `mambatrain.mamba2_layer`."""

    def __init__(self, d_model: int, d_state: int = 128, d_conv: int = 4, expand: int = 2, headdim: int = 64):
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand, self.headdim = d_model, d_state, d_conv, expand, headdim
        self.d_inner = expand * d_model
        self.nheads = self.d_inner // headdim
        conv_dim = self.d_inner + 2 * d_state
        self.in_proj = nn.Linear(d_model, 2 * self.d_inner + 2 * d_state + self.nheads, bias=False)
        self.conv1d = nn.Conv1d(conv_dim, conv_dim, d_conv, groups=conv_dim, padding=d_conv - 1, bias=True)
        dt = torch.exp(torch.rand(self.nheads) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3)).clamp(min=1e-4)
        self.dt_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))
        self.A_log = nn.Parameter(torch.log(torch.empty(self.nheads).uniform_(1.0, 16.0)))
        self.D = nn.Parameter(torch.ones(self.nheads))
        self.norm = _Norm(self.d_inner)
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=False)


def _check_shape(vocab_size, d_model, d_state, d_conv, expand, headdim, number_of_classes, padding_idx):
    ok = (vocab_size == VOCAB and number_of_classes == 2 and padding_idx == PAD and headdim == HEADDIM and d_conv == D_CONV
          and d_state in (16, 32, 64, 128) and d_model in (256, 512) and isinstance(expand, int) and expand >= 1
          and (expand * d_model) % 64 == 0)
    if not ok:
        raise NotImplementedError("the MI355X Mamba nets implement vocab 12, 2 classes, padding_idx 4, headdim 64, d_conv 4, "
                                  "d_state 16 / 32 / 64 / 128, embedding_dim 256 or 512 and an integer expand (configs/model/"
                                  "mamba.yaml, mambasp.yaml)")


class _MambaNet(nn.Module):
    _variant = None

    def _setup(self, d_model, n_layers, d_state, expand, headdim, max_len, precision, trajectory_stride=None, trainable=False):
        if precision not in ("fp32", "fp16x3"):
            raise ValueError("precision must be fp32 (exact fp32 products) or fp16x3 (every projection operand as two halfs, three "
                             "fp16 MFMAs per product: fp32-class logits)")
        self.precision = precision
        self.precision_report: dict = {}
        self._shape = (d_model, n_layers, d_state, expand, headdim, max_len)
        self._h, self._h32, self._last_h, self._dev, self._sig, self._hprec = None, None, None, None, None, None
        # the running verdict (an engine knob, csrc/mamba_verdict.hip): see the module docstring
        self.trajectory_stride = None if trajectory_stride is None else check_trajectory_stride(trajectory_stride)
        self.last_trajectory = None
        # training (mambatrain.py): with `trainable`, in train() and under autograd the forward builds a graph to every parameter
        self.trainable = bool(trainable)
        self._train = None
        self.last_train_pooled, self.last_train_route = None, None   # of the last training forward: pooled [B, d], the max-pool's positions

    def train_engine(self, device: torch.device):
        """The module's training engine on `device` (mambatrain.MambaTrainEngine), made on first use."""
        from .mambatrain import MambaTrainEngine

        if self._train is None or self._train.device != device:
            if self._train is not None:
                self._train.close()
            self._train = MambaTrainEngine(device)
        return self._train

    def trajectory_request(self):
        """The `engine.TrajectoryRequest` this module's forwards make (None: `trajectory_stride` is not set)."""
        return None if self.trajectory_stride is None else TrajectoryRequest(stride=self.trajectory_stride, summary=True)

    def _layer(self, i) -> Mamba2:
        raise NotImplementedError

    # ------------------------------------------------------------------ engine plumbing
    def _check(self, h, rc: int):
        if rc != 0:
            raise MambaEngineError(N.load().clm_mamba_last_error(h).decode())

    def _arith(self) -> str:
        """The arithmetic the loaded weights allow: fp16x3 only while every projection weight is inside its packing's range."""
        layers = [self._layer(i) for i in range(self._shape[1])]
        ws = [m.in_proj.weight for m in layers] + [m.out_proj.weight * m.norm.weight for m in layers]
        if hasattr(self, "input_block"):
            ws.append(self.input_block[0].weight)
        self.precision_report = x3_range_report(type(self).__name__, self.precision, ws)
        return self.precision_report.get("fallback_precision", self.precision)

    def _new_handle(self, lib, device: torch.device, prec: str):
        d, nl, ds, ex, hd, ml = self._shape
        h = C.c_void_p()
        dev = device.index if device.index is not None else torch.cuda.current_device()
        if lib.clm_mamba_create(dev, self._variant, N.PRECISIONS[prec], d, nl, ds, ex, hd, ml or 0, C.byref(h)) != 0:
            raise MambaEngineError(lib.clm_mamba_last_error(None).decode())
        N.upload_state_dict(self.state_dict().items(), partial(lib.clm_mamba_load_weight, h), partial(self._check, h))
        self._check(h, lib.clm_mamba_finalize(h))
        return h

    def _prepare(self, device: torch.device):
        # (not `_engine`: predict.py's end-of-run device check reads `net._engine` as the Hyena engine object)
        lib = N.load()
        sig = reload_signature(self)
        if self._h is not None and self._dev == device and sig == self._sig:
            return lib
        prec = self._arith()
        self.close()
        try:
            self._h = self._new_handle(lib, device, prec)
        except Exception:
            self.close()
            raise
        self._dev, self._hprec, self._sig = device, prec, sig
        return lib

    def refresh_weights(self) -> None:
        """The next forward rebuilds the handles from this module's tensors: for edits the signature cannot see (`p.data.mul_()`)."""
        self._sig = None

    def _run(self, lib, h, ids, dt, mask, out, req=None):
        """One forward of handle `h` into `out`; with a trajectory request also its `engine.TrajectoryOutput` (else None)."""
        B, L = ids.shape
        mptr = C.c_void_p(mask.data_ptr()) if mask is not None else None
        mstride = mask.stride(0) if mask is not None else 0
        trj, ct = trajectory_out(req, B, L, ids.device)
        self._check(h, lib.clm_mamba_forward_traj(h, C.c_void_p(ids.data_ptr()), dt, ids.stride(0), B, L, mptr, mstride,
                                                  C.c_void_p(out.data_ptr()), ct,
                                                  C.c_void_p(torch.cuda.current_stream(ids.device).cuda_stream)))
        return trj

    def _forward(self, input_ids: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
        if input_ids.device.type != "cuda":
            raise RuntimeError(f"chimeralm_amd.{type(self).__name__} runs on an MI355X only; there is no CPU forward")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32, torch.uint8):
            raise ValueError("input_ids must be [batch, length] of int64 / int32 / uint8")
        B, L = input_ids.shape
        if B == 0 or L == 0:
            raise ValueError(f"input_ids must hold at least one token of one read, got shape {tuple(input_ids.shape)}")
        max_len = self._shape[5]
        if max_len is not None and L > max_len:
            raise ValueError(f"read length {L} exceeds model_max_length {max_len} (the positional embedding's length)")
        if input_ids.stride(1) != 1:
            input_ids = input_ids.contiguous()
        if mask is not None:
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"the mask must be [batch, length] = {(B, L)}, got {tuple(mask.shape)}")
            mask = mask.to(device=input_ids.device, dtype=torch.float32)
            if mask.stride(1) != 1:
                mask = mask.contiguous()
        if self.trainable and self.training and torch.is_grad_enabled():
            from .mambatrain import train_forward

            return train_forward(self, input_ids, mask)
        lib = self._prepare(input_ids.device)
        dt = IDS_DT[input_ids.dtype]
        out = torch.empty((B, self.number_of_classes), dtype=torch.float32, device=input_ids.device)
        req = self.trajectory_request()
        self.last_trajectory = self._run(lib, self._h, input_ids, dt, mask, out, req)
        self._last_h = self._h
        if self._hprec == "fp16x3" and not bool(torch.isfinite(out).all()):
            # an activation outside fp16x3's range (the kernels return NaN for it): this batch again on the exact-fp32 kernels
            if self._h32 is None:
                self._h32 = self._new_handle(lib, input_ids.device, "fp32")
            self.last_trajectory = self._run(lib, self._h32, input_ids, dt, mask, out, req)
            self._last_h = self._h32
            self.precision_report["nonfinite_reruns"] = self.precision_report.get("nonfinite_reruns", 0) + 1
            _LOG.warning(f"chimeralm_amd: {type(self).__name__} fp16x3 returned non-finite logits (an activation beyond fp16's "
                         f"range); the batch of {B} reads was rerun on the exact-fp32 kernels")
        return out

    def debug_fetch(self, name: str, shape) -> np.ndarray:
        """Intermediates of the last forward, from the handle whose logits it returned (the exact-fp32 one after a non-finite
        fp16x3 rerun): "front" / "layer0" [B, L, d], "pooled" [B, d]; and, after a forward that ran as one chunk of reads, the LAST
        layer's workspace: "zx" [B, L, n_in_pad], "xc" [B, L, conv_dim], "g" [B, L, d_inner], "ssq" [B, L, H], "part" [B, ceil(L / 64),
        2, d] (include/chimeralm_hip.h)."""
        arr = np.empty(shape, dtype=np.float32)
        h = self._last_h
        self._check(h, N.load().clm_mamba_debug_fetch(h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def close(self):
        if getattr(self, "_train", None) is not None:
            self._train.close()
            self._train = None
        for attr in ("_h", "_h32"):
            h = getattr(self, attr, None)
            if h is not None:
                N.load().clm_mamba_destroy(h)
                setattr(self, attr, None)
        self._sig, self._last_h = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MambaSequenceClassification(_MambaNet):
    """The reference's `mamba` net: Embedding + pos_embedding -> Linear -> LayerNorm, Mamba2 layers with residuals, mean + max
    pooling, pooler, classifier.  forward(x, attention_mask=None)."""
    _variant = N.MAMBA_SEQ

    def __init__(self, vocab_size, embedding_dim: int, number_of_layers: int, model_max_length: int, dropout: float,
                 number_of_classes: int, d_state: int = 128, d_conv: int = 4, expand: int = 2, headdim: int = 64,
                 padding_idx: int = 4, *, precision: str = "fp16x3", trajectory_stride: int | None = None,
                 trainable: bool = False):
        super().__init__()
        _check_shape(vocab_size, embedding_dim, d_state, d_conv, expand, headdim, number_of_classes, padding_idx)
        self._setup(embedding_dim, number_of_layers, d_state, expand, headdim, model_max_length, precision, trajectory_stride, trainable)
        self.number_of_classes = number_of_classes
        self.embedding = nn.Embedding(vocab_size, embedding_dim, padding_idx=padding_idx)
        self.pos_embedding = nn.Parameter(torch.zeros(1, model_max_length, embedding_dim))
        self.input_block = nn.Sequential(nn.Linear(embedding_dim, embedding_dim), nn.LayerNorm(embedding_dim), nn.Dropout(dropout))
        self.mamba_layers = nn.ModuleList([nn.ModuleDict({"mamba": Mamba2(embedding_dim, d_state, d_conv, expand, headdim),
                                                          "dropout": nn.Dropout(dropout)}) for _ in range(number_of_layers)])
        self.pooler = nn.Sequential(nn.Linear(embedding_dim, embedding_dim), nn.GELU(), nn.Dropout(dropout))
        self.classifier = nn.Sequential(nn.Linear(embedding_dim, embedding_dim // 2), nn.GELU(), nn.Dropout(dropout),
                                        nn.Linear(embedding_dim // 2, number_of_classes))
        nn.init.normal_(self.pos_embedding, std=0.02)

    def _layer(self, i) -> Mamba2:
        return self.mamba_layers[i]["mamba"]

    def forward(self, x: torch.Tensor, attention_mask: torch.Tensor | None = None) -> torch.Tensor:
        return self._forward(x, attention_mask)


class MambaSequenceClassificationSP(_MambaNet):
    """The reference's `mambasp` net: Embedding, Mamba2 layers with residuals, mean + max pooling, pooler, classifier.
    forward(input_ids, input_quals=None); `input_quals` is accepted and ignored, as in the reference."""
    _variant = N.MAMBA_SP

    def __init__(self, vocab_size, embedding_dim: int, number_of_layers: int, number_of_classes: int, dropout: float,
                 d_state: int = 128, d_conv: int = 4, expand: int = 2, headdim: int = 64, padding_idx: int = 4, *,
                 precision: str = "fp16x3", trajectory_stride: int | None = None, trainable: bool = False):
        super().__init__()
        _check_shape(vocab_size, embedding_dim, d_state, d_conv, expand, headdim, number_of_classes, padding_idx)
        self._setup(embedding_dim, number_of_layers, d_state, expand, headdim, None, precision, trajectory_stride, trainable)
        self.number_of_classes = number_of_classes
        self.embedding = nn.Embedding(vocab_size, embedding_dim, padding_idx=padding_idx)
        self.mamba_layers = nn.ModuleList([Mamba2(embedding_dim, d_state, d_conv, expand, headdim) for _ in range(number_of_layers)])
        self.pooler = nn.Sequential(nn.Linear(embedding_dim, embedding_dim), nn.GELU(), nn.Dropout(dropout))
        self.classifier = nn.Sequential(nn.Linear(embedding_dim, embedding_dim // 2), nn.GELU(), nn.Dropout(dropout),
                                        nn.Linear(embedding_dim // 2, number_of_classes))

    def _layer(self, i) -> Mamba2:
        return self.mamba_layers[i]

    def forward(self, input_ids: torch.Tensor, input_quals: torch.Tensor | None = None) -> torch.Tensor:
        return self._forward(input_ids, None)
