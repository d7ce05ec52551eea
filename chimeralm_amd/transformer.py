"""Drop-in for the reference's second net, `SequenceCNNTransformer`
(/root/reference/chimeralm/models/components/transformer.py:28-104, configs/model/transformer.yaml:3-12), with the forward on MI355X.

Same constructor arguments, same `state_dict()` keys (torch's own modules are used as parameter containers, so
`transformer_encoder.layers.{i}.self_attn.in_proj_weight` etc. come out exactly as in the reference, and `pos_encoder.pe` is a
buffer of the same shape), same `forward(input_ids, input_quals=None) -> logits [B, 2]`, same `number_of_classes` attribute that
`ClassificationLit` reads.  The arithmetic runs in csrc/tf_model.hip + csrc/attention.hip behind the `clm_tf_*` C ABI; there is no
CPU path.  Engine knobs absent in the reference: `precision` in {"fp32", "fp16x3", "fp16c", "fp16", "bf16"} -- fp32 = the
reference's arithmetic; **fp16x3 (the default)** = every operand as two halfs, three fp16 MFMAs per product: 7e-6 .. 2.2e-5 from the
reference module on the cases it was run on, 2.3x the exact rate, unguarded; fp16c = fp16 activations x weights as fp16 hi + fp8
lo, the Hyena path's compensated mode: twice fp16x3's rate, but 2e-3 from the reference on those cases -- outside its 1e-3
tolerance there, so it is opt-in and guarded (HISTORY.md section 5b) -- and `selfcheck` / `selfcheck_tol`: before the first batch
after a weight load (and again every `selfcheck_every`-th batch, for a batch more than 1.5x shorter or longer than any checked so
far, and for the batch after a measurement within 10 % of the threshold) the mode is measured against the exact-fp32 kernels of the
same engine on seeded reads and on rows of the batch (`clm_tf_selfcheck`); above the threshold the module falls back for good --
a 16-bit mode to fp16x3, the next-fastest arithmetic inside the tolerance (`clm_tf_set_fallback` level 1), fp16x3 to exact fp32 --
and says so.  On by default for fp16c.  WHICH batches are measured is the rule `HyenaDna` follows too, kept in `self._guard`
(`_guard.GuardSchedule`, reset by every weight load); this module's own are its one seeded sample and its verdict.  fp16x3 -- the
default mode, and the first fall-back level of the 16-bit modes -- packs weights x 2^10 as fp16 halfs, which saturate at
|w| >= 64: if a CNN-stem or encoder weight is that large (or NaN), the engine runs exact fp32 wherever it would run fp16x3; the
module reads that back at every weight load (`clm_tf_effective_precision`), records it in `precision_report` and logs a warning.

Training (`trainable=True`, keyword-only; tftrain.py): in `train()` mode and with autograd on, `forward` builds a
graph to every parameter in exact fp32 -- the attention core forward and backward on the engine (`attention_core="engine"`,
csrc/attention_train.hip) or through `F.scaled_dot_product_attention` (`"torch"`), everything around it in torch.  Every other call
is the inference forward above, bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math
from functools import partial

import numpy as np
import torch
from torch import nn

from . import _native as N
from ._guard import GuardSchedule, announce_fallback, finite_or_inf, sample_rows, x3_range_report
from ._reload import reload_signature
from .engine import IDS_DT

_X3_PACKED = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight", "cnn.0.weight",
              "cnn.3.weight", "cnn.6.weight")


class _PosEnc(nn.Module):
    def __init__(self, d_model: int, max_len: int):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))


class TransformerEngineError(RuntimeError):
    pass


class SequenceCNNTransformer(nn.Module):
    def __init__(self, vocab_size: int, max_len: int, d_model: int = 256, cnn_kernel_size: int = 3, dropout: float = 0.1,
                 num_encoder_layers: int = 2, nhead: int = 8, dim_feedforward: int = 1024, number_of_classes: int = 2,
                 padding_idx: int = 4, *, precision: str = "fp16x3", selfcheck: bool | None = None, selfcheck_tol: float = 5e-4,
                 selfcheck_every: int = 16, trainable: bool = False, attention_core: str = "engine"):
        super().__init__()
        if (vocab_size, d_model, cnn_kernel_size, nhead, dim_feedforward, number_of_classes) != (12, 256, 3, 8, 1024, 2):
            raise NotImplementedError("the MI355X encoder implements the production shape: vocab 12, d_model 256, kernel 3, "
                                      "8 heads, feed-forward 1024, 2 classes (configs/model/transformer.yaml)")
        if precision not in ("fp32", "fp16x3", "fp16c", "fp16", "bf16"):
            raise ValueError("precision must be fp32 (exact fp32 products: the reference's arithmetic, the parity mode), fp16x3 "
                             "(every operand as two halfs, three fp16 MFMAs per product: fp32-class accuracy at 2.5x the rate), fp16c "
                             "(fp16 activations x hi + lo weights, self-checked) or fp16 / bf16 (plain 16-bit MFMA inputs, fp32 "
                             "accumulation and statistics: reduced precision)")
        self.number_of_classes, self.precision, self.num_encoder_layers = number_of_classes, precision, num_encoder_layers
        self.selfcheck = (precision == "fp16c") if selfcheck is None else bool(selfcheck)
        self.selfcheck_tol = float(selfcheck_tol)
        self.selfcheck_report: dict = {}
        self.precision_report: dict = {}
        self.selfcheck_every = int(selfcheck_every)
        self._guard = GuardSchedule(self.selfcheck_tol, self.selfcheck_every)   # (`heard` here: something was measured)
        self.embedding = nn.Embedding(vocab_size, d_model, padding_idx=padding_idx)
        self.pos_encoder = _PosEnc(d_model, max_len)
        conv = lambda: nn.Conv1d(d_model, d_model, kernel_size=cnn_kernel_size, padding=1)  # noqa: E731
        self.cnn = nn.Sequential(conv(), nn.ReLU(), nn.MaxPool1d(2, 2), conv(), nn.ReLU(), nn.MaxPool1d(2, 2), conv(), nn.ReLU(),
                                 nn.MaxPool1d(2, 2))
        self.norm = nn.LayerNorm(d_model)
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                                           batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_encoder_layers, enable_nested_tensor=False)
        self.attn_pool = nn.Linear(d_model, 1)
        self.classifier = nn.Sequential(nn.Linear(d_model, d_model // 2), nn.ReLU(), nn.Dropout(dropout),
                                        nn.Linear(d_model // 2, number_of_classes))
        self._h, self._dev, self._sig = None, None, None
        self._stop = -1                                        # debug_stop_after
        # training (tftrain.py): with `trainable`, in train() and under autograd the forward builds a graph to every parameter, in
        # exact fp32 whatever `precision` says; `attention_core` = "engine" (csrc/attention_train.hip) or "torch" (the comparison path)
        if attention_core not in ("engine", "torch"):
            raise ValueError('attention_core must be "engine" (the HIP op) or "torch" (F.scaled_dot_product_attention)')
        self.trainable, self.attention_core, self.dropout = bool(trainable), attention_core, float(dropout)
        self._dropout_generator, self._attn_draws = None, 0

    @property
    def dropout_generator(self):
        """The generator of the training forward's dropout masks (None: torch's default one).  Assigning one restarts the stream of
        attention seeds: two nets given equally seeded generators draw the same masks."""
        return self._dropout_generator

    @dropout_generator.setter
    def dropout_generator(self, gen):
        self._dropout_generator, self._attn_draws = gen, 0

    def next_attention_seed(self) -> int:
        """The 64-bit seed of the next attention call: host arithmetic on the generator's seed and a call counter, so that drawing it
        never waits for the device."""
        from .tftrain import layer_seed

        gen = self._dropout_generator
        base = gen.initial_seed() if gen is not None else torch.initial_seed()
        self._attn_draws += 1
        return layer_seed(base, self._attn_draws - 1)

    # ------------------------------------------------------------------ engine plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise TransformerEngineError(N.load().clm_tf_last_error(self._h).decode())

    def _engine(self, device: torch.device):
        lib = N.load()
        if self._h is None or self._dev != device:
            self.close()
            h = C.c_void_p()
            rc = lib.clm_tf_create(device.index if device.index is not None else torch.cuda.current_device(), N.PRECISIONS[self.precision], self.num_encoder_layers, C.byref(h))
            if rc != 0:
                raise TransformerEngineError(lib.clm_tf_last_error(None).decode())
            self._h, self._dev, self._sig = h, device, None
            if self._stop >= 0:
                self._check(lib.clm_tf_debug_stop_after(self._h, self._stop))
        sig = reload_signature(self)
        if sig != self._sig:                                   # weights replaced or modified in place -> reload
            N.upload_state_dict(self.state_dict().items(), partial(lib.clm_tf_load_weight, self._h), self._check)
            self._check(lib.clm_tf_finalize(self._h))
            self._check(lib.clm_tf_set_fallback(self._h, 0))
            self._sig, self.selfcheck_report = sig, {}
            self._guard.reset()
            self._report_x3(lib)
        return lib

    def refresh_weights(self) -> None:
        """The next forward reloads the engine from this module's tensors: for edits the signature cannot see (`p.data.mul_()`)."""
        self._sig = None

    def _arith(self, lib) -> str:
        """The arithmetic the engine runs a forward in right now (`clm_tf_effective_precision`)."""
        code = lib.clm_tf_effective_precision(self._h)
        if code < 0:
            raise TransformerEngineError(f"clm_tf_effective_precision: error {code}")
        return N.PREC_NAMES[code]

    def _report_x3(self, lib) -> None:
        """`precision_report` of the weights just loaded: what the engine runs where this mode uses fp16x3 (its own mode; the first
        fall-back level of a 16-bit mode), read back from it, and a warning when the weights pushed it to exact fp32."""
        if self.precision == "fp32":
            x3 = None
        elif self.precision == "fp16x3":
            x3 = self._arith(lib)
        else:
            self._check(lib.clm_tf_set_fallback(self._h, 1))
            x3 = self._arith(lib)
            self._check(lib.clm_tf_set_fallback(self._h, 0))
        where = "" if self.precision == "fp16x3" else " (its first fall-back level)"
        self.precision_report = x3_range_report(
            "SequenceCNNTransformer", self.precision, (t for k, t in self.state_dict().items() if k.endswith(_X3_PACKED)),
            effective=x3, where=f" for fp16x3{where}", tail="it runs the exact-fp32 kernels there")

    # ------------------------------------------------------------------ the 16-bit mode on trial
    def _selfcheck_call(self, lib, ids: torch.Tensor) -> tuple[float, int]:
        """`clm_tf_selfcheck` on `ids`: the largest logit difference between the mode and exact fp32, and whether a label differs."""
        diff, differ = C.c_float(), C.c_int()
        self._check(lib.clm_tf_selfcheck(self._h, C.c_void_p(ids.data_ptr()), IDS_DT[ids.dtype], ids.stride(0), ids.shape[0],
                                         ids.shape[1], C.c_void_p(torch.cuda.current_stream(ids.device).cuda_stream), C.byref(diff),
                                         C.byref(differ)))
        return diff.value, differ.value

    def _measure(self, lib, name: str, ids: torch.Tensor) -> float:
        diff, differ = self._selfcheck_call(lib, ids)
        self.selfcheck_report.setdefault("samples", []).append({"sample": name, "max_abs_dlogit": diff, "labels_differ": differ})
        return diff

    def guard_due(self, n_tokens: int) -> bool:
        """Is a self-check due for a batch of `n_tokens`-token reads (`GuardSchedule.due`)?  Never without `selfcheck`, in fp32 or once
        fallen back.  No length switch here (every batch is on trial) and no wait for reads.  Counts the batch."""
        if not self.selfcheck or self.precision == "fp32" or self.selfcheck_report.get("fallback"):
            return False
        self._guard.tol, self._guard.every = self.selfcheck_tol, self.selfcheck_every   # as they are NOW: assignable after construction
        return self._guard.due(n_tokens)

    def guard(self, lib, input_ids: torch.Tensor) -> None:
        """Self-check of the 16-bit mode where one is due (see the module docstring)."""
        rep, L = self.selfcheck_report, input_ids.shape[1]
        if not self.guard_due(L):
            return
        sched, now = self._guard, 0.0
        if not sched.heard:                                    # first batch since the weights were loaded: ONE seeded sample,
            g = torch.Generator().manual_seed(20241)           # without [SEP], and no second level behind it
            Ls = min(4096, 8 * self.pos_encoder.pe.shape[1])   # (a model built with a short max_len cannot take 4,096 tokens)
            ids = torch.randint(7, 11, (4, Ls), generator=g, dtype=torch.uint8)
            ids[0, : Ls // 3] = 4                              # one read left-padded, as the collator pads
            now = max(now, self._measure(lib, f"synthetic 4 x {Ls}", ids.to(input_ids.device)))
        rows = sample_rows(input_ids.shape[0], 4)
        now = finite_or_inf(max(now, self._measure(lib, f"batch rows {rows} x {L}", input_ids[rows].contiguous())))
        worst = max(rep.get("max_abs_dlogit", 0.0), now)       # the verdict is taken on the running maximum, the re-arm on `now`
        rep.update(max_abs_dlogit=worst, tol=self.selfcheck_tol, precision=self.precision)
        sched.record(L, now)                                   # every check widens the range; no `checks` counter
        if not worst <= self.selfcheck_tol:                    # (NaN fails too)
            self._check(lib.clm_tf_set_fallback(self._h, 1))
            announce_fallback(rep, subject="SequenceCNNTransformer ", precision=self.precision, worst=worst, tol=self.selfcheck_tol,
                              fallback_precision=self._arith(lib))
        rep.setdefault("fallback", False)

    def forward(self, input_ids: torch.Tensor, input_quals: torch.Tensor | None = None) -> torch.Tensor:
        """`input_quals` is accepted and ignored, as in the reference (transformer.py:88)."""
        if input_ids.device.type != "cuda":
            raise RuntimeError("chimeralm_amd.SequenceCNNTransformer runs on an MI355X only; there is no CPU forward")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32, torch.uint8):
            raise ValueError("input_ids must be [batch, length] of int64 / int32 / uint8")
        if input_ids.stride(1) != 1:
            input_ids = input_ids.contiguous()
        if self.trainable and self.training and torch.is_grad_enabled():
            from .tftrain import train_forward

            return train_forward(self, input_ids)
        lib = self._engine(input_ids.device)
        self.guard(lib, input_ids)
        B, L = input_ids.shape
        out = torch.empty((B, 2), dtype=torch.float32, device=input_ids.device)
        self._check(lib.clm_tf_forward(self._h, C.c_void_p(input_ids.data_ptr()), IDS_DT[input_ids.dtype], input_ids.stride(0), B, L,
                                       C.c_void_p(out.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(input_ids.device).cuda_stream)))
        return out

    TF_STAGES = ("conv_stack_pe_ln", "attention", "encoder_layer", "pool_head")

    def profile_enable(self, on: bool = True):
        self._check(N.load().clm_tf_profile_enable(self._h, int(on)))

    def profile_read(self, reset: bool = True) -> dict[str, tuple[float, int]]:
        ms, n = (C.c_double * 4)(), (C.c_int64 * 4)()
        self._check(N.load().clm_tf_profile_read(self._h, ms, n, int(reset)))
        return {self.TF_STAGES[i]: (ms[i], n[i]) for i in range(4)}

    # the launches of a forward, in order: include/chimeralm_hip.h CLM_TF_STAGE_*, CLM_TF_STAGE_ATTENTION(i) and CLM_TF_STAGE_LAYER(i)
    # (tests/test_tf_stage_host.py compares these with the header); ("attention", i) and ("layer", i) per layer
    TF_STOPS = {"embed": 0, "conv1": 1, "conv2": 2, "conv3": 3, "pe_ln": 4, "in_proj": 5}
    _STOP_ATTENTION0, _STOP_LAYER0, _STOP_PER_LAYER = 6, 7, 2

    def debug_stop_after(self, stage=None) -> None:
        """Tests only: every later forward returns right after the launch `stage` -- a name of TF_STOPS, ("attention", i) or
        ("layer", i) -- and launches nothing behind it (the returned logits are then uninitialised); None: whole forwards again.
        Set before the first forward it takes effect when the engine is created."""
        if stage is None:
            code = -1
        elif isinstance(stage, tuple):
            code = {"attention": self._STOP_ATTENTION0, "layer": self._STOP_LAYER0}[stage[0]] + self._STOP_PER_LAYER * int(stage[1])
        else:
            code = self.TF_STOPS[stage]
        if self._h is not None:
            self._check(N.load().clm_tf_debug_stop_after(self._h, code))
        self._stop = code

    def debug_fetch(self, name: str, shape, dtype=np.float32) -> np.ndarray:
        """A buffer of the last forward (names and shapes: include/chimeralm_hip.h).  The 16-bit path's activations are raw bits:
        fetch them as np.uint16 (bf16) or np.float16."""
        arr = np.empty(shape, dtype=dtype)
        self._check(N.load().clm_tf_debug_fetch(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def close(self):
        if getattr(self, "_h", None) is not None:
            N.load().clm_tf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
