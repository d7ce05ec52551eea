"""Host-side mirror of the reference's `net` for the predict path.

Mirrors /root/reference/chimeralm/models/components/hyena.py:
  `HyenaDna(number_of_classes, head, backbone_name, *, freeze_backbone)`  (:218-242)
  `HyenaDna.forward(input_ids, input_quals=None) -> logits[B, 2]`         (:244-256)
  `BinarySequenceClassifier`, `ResidualBlock`                             (:6-180)
with the same constructor arguments, attribute names and `state_dict()` keys, so checkpoints written
by the reference load unchanged (`net.backbone.backbone.layers.0.mixer.in_proj.weight`, ...).

The modules here only OWN parameters.  All arithmetic runs in the MI355X engine behind the C ABI
(`chimeralm_amd.engine.Engine`); there is no PyTorch or CPU forward -- calling `forward` without the
HIP library or with CPU tensors raises.
"""
from __future__ import annotations

import logging
import math

import torch
from torch import nn

from ._guard import GuardSchedule, announce_fallback, finite_or_inf, sample_rows, x3_range_report
from ._reload import reload_signature
from .engine import Engine, check_trajectory_stride

_X3_PACKED = ("mixer.in_proj.weight", "mixer.out_proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "head.attention.0.weight")
_SMALL_32K = dict(d_model=256, n_layer=4, d_inner=1024, vocab_rows=16, filter_order=64, emb_dim=5, max_seq_len=32770)


class _Holder(nn.Module):
    """Parameter container; never executed."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container of the MI355X engine: use HyenaDna.forward")


def _linear(out_f: int, in_f: int, bias: bool = True) -> nn.Linear:
    return nn.Linear(in_f, out_f, bias=bias)  # default init; used as a container only


class _Sin(_Holder):
    def __init__(self, width: int, freq: float = 10.0):
        super().__init__()
        self.freq = nn.Parameter(freq * torch.ones(1, width))


class _PosEmb(_Holder):
    def __init__(self, emb_dim: int, seq_len: int):
        super().__init__()
        t = torch.linspace(0, 1, seq_len, dtype=torch.float64)[None, :, None]
        bands = (emb_dim - 1) // 2
        w = 2 * math.pi * torch.linspace(0, seq_len - 1, seq_len, dtype=torch.float64)[None, :, None] / seq_len
        f = torch.linspace(1e-4, bands - 1, bands, dtype=torch.float64)[None, None]
        z = torch.exp(-1j * f * w)
        self.z = nn.Parameter(torch.cat([t, z.real, z.imag], dim=-1).float())
        self.register_buffer("t", t.float())


class _Modulation(_Holder):
    def __init__(self, d_model: int, fast=0.3, slow=1.5, target=1e-2):
        super().__init__()
        deltas = torch.linspace(math.log(target) / slow, math.log(target) / fast, d_model, dtype=torch.float64)
        self.register_buffer("deltas", deltas[None, None].float())


class _Filter(_Holder):
    def __init__(self, c):
        super().__init__()
        self.bias = nn.Parameter(torch.randn(c["d_model"]))
        self.pos_emb = _PosEmb(c["emb_dim"], c["max_seq_len"])
        act = _Sin(c["filter_order"])          # ONE module registered three times (keys .1/.3/.5 .freq)
        self.implicit_filter = nn.Sequential(
            _linear(c["filter_order"], c["emb_dim"]), act,
            _linear(c["filter_order"], c["filter_order"]), act,
            _linear(c["filter_order"], c["filter_order"]), act,
            _linear(c["d_model"], c["filter_order"], bias=False),
        )
        self.modulation = _Modulation(c["d_model"])


class _Mixer(_Holder):
    def __init__(self, c):
        super().__init__()
        d = c["d_model"]
        self.in_proj = _linear(3 * d, d)
        self.out_proj = _linear(d, d)
        self.short_filter = nn.Conv1d(3 * d, 3 * d, 3, padding=2, groups=3 * d)
        self.filter_fn = _Filter(c)


class _Mlp(_Holder):
    def __init__(self, c):
        super().__init__()
        self.fc1 = _linear(c["d_inner"], c["d_model"])
        self.fc2 = _linear(c["d_model"], c["d_inner"])


class _Block(_Holder):
    def __init__(self, c):
        super().__init__()
        self.mixer = _Mixer(c)
        self.norm1 = nn.LayerNorm(c["d_model"], eps=1e-5)
        self.mlp = _Mlp(c)
        self.norm2 = nn.LayerNorm(c["d_model"], eps=1e-5)


class _Embeddings(_Holder):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c["vocab_rows"], c["d_model"])


class _LMBackbone(_Holder):
    def __init__(self, c):
        super().__init__()
        self.embeddings = _Embeddings(c)
        self.layers = nn.ModuleList([_Block(c) for _ in range(c["n_layer"])])
        self.ln_f = nn.LayerNorm(c["d_model"], eps=1e-5)


class HyenaDNAParams(_Holder):
    """Parameter tree with the key layout of the HF model `LongSafari/hyenadna-small-32k-seqlen-hf`
    (`HyenaDNAModel.backbone.*`), which the reference builds at hyena.py:237."""

    def __init__(self, backbone_name: str = "hyenadna-small-32k-seqlen"):
        super().__init__()
        if backbone_name != "hyenadna-small-32k-seqlen":
            raise NotImplementedError(
                f"backbone {backbone_name!r}: the MI355X engine is built for hyenadna-small-32k-seqlen, the only "
                "backbone `chimeralm predict` uses (chimeralm/models/lm.py:21)")
        self.backbone = _LMBackbone(_SMALL_32K)


# ------------------------------------------------------------------------------------------------ head
class ResidualBlock(_Holder):
    """Parameters of the reference's ResidualBlock (hyena.py:149-180)."""

    def __init__(self, hidden_dim: int, dropout: float = 0.1):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.GELU(), nn.Dropout(dropout),
                                    nn.Linear(hidden_dim, hidden_dim))
        self.dropout = nn.Dropout(dropout)


class BinarySequenceClassifier(_Holder):
    """Parameters and hyper-parameters of the reference head (hyena.py:16-77); same constructor."""

    def __init__(self, input_dim: int, hidden_dim: int = 512, num_layers: int = 2, dropout: float = 0.1,
                 pooling_type: str = "attention", activation: str = "gelu", *, use_residual: bool = True,
                 save_attention: bool = False):
        super().__init__()
        if (input_dim, hidden_dim, num_layers, pooling_type, activation, use_residual) != (256, 512, 2, "attention",
                                                                                           "gelu", True):
            raise NotImplementedError(
                "the MI355X engine implements the production head only: input_dim=256, hidden_dim=512, num_layers=2, "
                "pooling_type='attention', activation='gelu', use_residual=True (chimeralm/models/lm.py:22-31)")
        self.input_dim, self.hidden_dim, self.pooling_type = input_dim, hidden_dim, pooling_type
        self.use_residual, self.save_attention = use_residual, save_attention
        self.activation = nn.GELU()
        self.attention = nn.Sequential(nn.Linear(input_dim, hidden_dim // 2), self.activation,
                                       nn.Linear(hidden_dim // 2, 1), nn.Softmax(dim=1))
        self.classifier = nn.Sequential(
            nn.Linear(input_dim, hidden_dim), self.activation, nn.Dropout(dropout),
            nn.Linear(hidden_dim, hidden_dim), self.activation, nn.Dropout(dropout),
            ResidualBlock(hidden_dim, dropout),
        )
        self.output_layer = nn.Linear(hidden_dim, 2)
        if save_attention:
            self.attention_weights = None


_HEAD_KEYS = ("attention.0.weight", "attention.0.bias", "attention.2.weight", "attention.2.bias",
              "classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias",
              "classifier.6.layers.0.weight", "classifier.6.layers.0.bias", "classifier.6.layers.3.weight",
              "classifier.6.layers.3.bias", "output_layer.weight", "output_layer.bias")


class HyenaDna(nn.Module):
    """Drop-in for the reference's `HyenaDna` net: same signature, same state_dict keys, MI355X forward.

    Extra keyword-only arguments (engine knobs, absent in the reference):
    `precision` selects the arithmetic of the dense projections -- "fp32" (exact, the reference's), "fp16x3" (every operand as two
    halfs, three fp16 MFMAs per product: fp32-class logits, ~1e-5 from exact, at about twice the exact rate), "fp16c" (fp16
    activations carried with one e5m2 lo byte x in_proj / out_proj / score weights held as fp16 hi + fp8 lo, MLP weights plain fp16:
    16-bit MFMA rate; 1.3e-4 median / 5.4e-4 max from the fp32 reference over the 32 seeded study batches; reads
    below `f16c_min_len` tokens -- 2,048 unless measured lower -- run in the fp16x3 kernels), "fp16" / "bf16" (reduced precision,
    outside the reference's 1e-3 tolerance); `chunk_reads` the number of reads pushed through all layers together.
    `selfcheck` (default: on for "fp16c") -- the reference runs ONE precision, fp32, always (hyena.py:244-256); a 16-bit mode's
    distance from it depends on the weights, so it is MEASURED on the weights actually loaded (`clm_selfcheck`: the same reads
    through the mode and through the exact-fp32 kernels of the same engine).  Before the first batch after every weight (re)load:
    seeded synthetic samples of 4,097, 2,048, 1,024, 512 and 256 tokens -- the shortest one that still passes (with every longer
    one) becomes the length below which reads take the fp16x3 kernels inside the mode (`clm_set_short_read_len`; 4,098 if not even
    the longest sample passes).  "Passes" = within `selfcheck_tol` (5e-4, half the tolerance) down to the unmeasured default of 2,048
    tokens and within HALF of it below: one seeded sample places the switch, so lowering it wants a margin of 2 -- and four reads
    spread over that batch.  Later: four reads of every `selfcheck_every`-th batch (16; and not before `selfcheck_min_reads` =
    1,024 reads went by, so that small batches do not pay 10 % for it), of any batch more than 1.5x shorter or
    longer than every batch measured so far, and of the batch that follows a measurement within 10 % of the threshold.  A sample,
    not a bound: batches in between are not measured.  A BATCH above the threshold moves fp16c to its second level -- its MLP
    products run on plain fp16 weights (fast; enough on most weights) and then on hi + lo weights like the other projections
    (`clm_set_mlp_compensation`, ~10 % slower), heard again from the start -- and only if that form fails on the batch too does the
    engine fall back for good (logged, RuntimeWarning): to fp16x3, the next-fastest arithmetic inside the gate
    (`clm_set_fallback` level 1; an "fp16x3" module that was asked to check itself falls back to exact fp32).  `selfcheck_report`
    holds what was measured; WHICH batches are measured is kept in `self._guard` (`_guard.GuardSchedule`: what was heard, the length
    range checked, the batches and reads since; shared with `SequenceCNNTransformer`), reset by every weight load.
    fp16x3 -- the "fp16x3" mode, fp16c's short reads and the first fall-back level of the 16-bit modes -- packs weights x 2^10 as
    fp16 halfs, which saturate at |w| >= 64: if an in_proj / out_proj / fc1 / fc2 / score weight is that large (or NaN), the engine
    runs exact fp32 wherever it would run fp16x3; the module reads that back at every weight load, records it in `precision_report`
    and logs a warning.
    """

    def __init__(self, number_of_classes: int, head: nn.Module, backbone_name: str = "hyenadna-small-32k-seqlen", *,
                 freeze_backbone: bool = False, precision: str = "fp16c", chunk_reads: int = 256,
                 selfcheck: bool | None = None, selfcheck_tol: float = 5e-4, selfcheck_every: int = 16,
                 attention_top_k: int | None = None, trajectory_stride: int | None = None, trainable: bool = False,
                 hyena_core: str = "engine", hyena_long_core: str = "torch"):
        super().__init__()
        if hyena_long_core not in ("torch", "engine"):
            raise ValueError('hyena_long_core must be "torch" (reads beyond 8,193 tokens train on conv1d and rfft / irfft) or "engine" '
                             "(the segmented HIP op up to 32,769 tokens, csrc/hyena_longtrain.hip)")
        if hyena_core not in ("engine", "torch"):
            raise ValueError('hyena_core must be "engine" (the HIP op, csrc/hyena_train.hip) or "torch" (conv1d and rfft / irfft)')
        if number_of_classes != 2:
            raise NotImplementedError("the engine implements the binary (2-class) head only")
        missing = [k for k in _HEAD_KEYS if k not in head.state_dict()]
        if missing or getattr(head, "pooling_type", "attention") != "attention":
            raise NotImplementedError(f"head is not the production attention-pooling classifier (missing {missing})")
        self.number_of_classes = number_of_classes
        self.backbone_name = backbone_name
        self.backbone = HyenaDNAParams(backbone_name)
        self.head = head
        self.precision = precision
        self.chunk_reads = chunk_reads
        self.selfcheck = (precision == "fp16c") if selfcheck is None else bool(selfcheck)
        self.selfcheck_tol = float(selfcheck_tol)
        self.selfcheck_every = int(selfcheck_every)
        self.selfcheck_report: dict = {}
        self.precision_report: dict = {}
        # attention as an output (an engine knob, csrc/attn_weights.hip): with `attention_top_k` set every forward also leaves
        # `last_attention`, an engine.AttentionOutput of DEVICE tensors -- per read the summary and its top-k bases, and the weights
        # of every position too when `attention_device_weights` is set (the predict loops set it for --attention-weights)
        self.attention_top_k = None if attention_top_k is None else int(attention_top_k)
        self.attention_device_weights = False
        self.last_attention = None
        # the running verdict (an engine knob, csrc/trajectory.hip): with `trajectory_stride` set every forward also leaves
        # `last_trajectory`, an engine.TrajectoryOutput of DEVICE tensors -- the logits the model would give if a row ended at each
        # multiple of the stride, and per read the summary (where the verdict settles, where it moves most)
        self.trajectory_stride = None if trajectory_stride is None else check_trajectory_stride(trajectory_stride)
        self.last_trajectory = None
        self.freeze_backbone = bool(freeze_backbone)
        if freeze_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False
        # training of the whole net (hyenatrain.py): with `trainable` and an unfrozen backbone, in train() and under
        # autograd, the forward builds a graph to every parameter, in exact fp32 whatever `precision` says.  `hyena_core`: the
        # operator's core on the engine or in torch; `embed_dropout`: the backbone's only dropout, on the embedding output, drawn from
        # `dropout_generator` (None: torch's default generator); `last_train_core`: the core the last training forward took.
        # `hyena_long_core`: with hyena_core="engine", where reads of 8,194 ... 32,769 tokens train -- "torch", or "engine": the segmented
        # op (last_train_core "engine-long")
        self.trainable, self.hyena_core, self.hyena_long_core = bool(trainable), hyena_core, hyena_long_core
        self.embed_dropout = 0.1
        self.dropout_generator = None
        self.last_train_core = None
        self._engine: Engine | None = None
        self._engine_sig = None
        # when the mode is measured again since the last weight load (`heard`: the seeded samples ran); knobs: `guard_due`
        self._guard = GuardSchedule(self.selfcheck_tol, self.selfcheck_every, self.selfcheck_min_reads)
        self._mlp_lo = False                              # fp16c: the guard's second level is on (fc1 / fc2 on hi + lo weights)

    # -------------------------------------------------------------------------------- engine plumbing
    def _signature(self):
        return reload_signature(self)

    def refresh_weights(self) -> None:
        """The next forward reloads the engine from this module's tensors: for edits the signature cannot see (`p.data.mul_()`)."""
        self._engine_sig = None

    def engine(self, device: torch.device) -> Engine:
        """Engine for `device`, (re)loaded whenever a parameter tensor was replaced or modified in place."""
        if self._engine is None or self._engine.device != device:
            if self._engine is not None:
                self._engine.close()
            self._engine = Engine(device, precision=self.precision, chunk_reads=self.chunk_reads)
            self._engine_sig = None
        sig = self._signature()
        if sig != self._engine_sig:
            self._engine.load_state_dict(self.state_dict())
            self._engine_sig = sig
            self._engine.set_fallback(False)               # new weights: the mode gets a new hearing ...
            if self.precision == "fp16c":
                self._engine.set_f16c_min_len(self._DEFAULT_MIN_LEN)   # ... the length switch its unmeasured default ...
                self._engine.set_mlp_compensation(False)   # ... and the MLP its plain-fp16 weights
            self._mlp_lo = False
            self._guard.reset()
            self.selfcheck_report = {}
            self._report_x3(self._engine)
        return self._engine

    def _report_x3(self, eng: Engine) -> None:
        """`precision_report` of the weights just loaded: the arithmetic the engine runs where this mode uses fp16x3 (see the class
        docstring), read back from the engine, and a warning when the weights pushed it to exact fp32."""
        if self.precision == "fp32":
            x3 = None
        elif self.precision in ("fp16x3", "fp16c"):           # its own mode / its short reads (level 0, one-token reads)
            x3 = eng.effective_precision(1)
        else:                                                 # fp16 / bf16: only their first fall-back level is fp16x3
            eng.set_fallback(1)
            x3 = eng.effective_precision(1)
            eng.set_fallback(0)
        where = {"fp16x3": "", "fp16c": " (its reads below f16c_min_len and its first fall-back level)"}.get(self.precision, " (its first fall-back level)")
        self.precision_report = x3_range_report(
            "HyenaDna", self.precision, (t for k, t in self.state_dict().items() if k.endswith(_X3_PACKED)), effective=x3,
            where=f" for fp16x3{where}", tail="it runs the exact-fp32 kernels there")

    # -------------------------------------------------------------------------------- the 16-bit mode on trial
    _SAMPLE_LENGTHS = (4097, 2048, 1024, 512, 256)       # descending: the mode's error grows like 1 / sqrt(L)
    _BATCH_ROWS = 4                                       # reads of a batch that a check runs through both arithmetics
    _DEFAULT_MIN_LEN = 2048                               # fp16c's length switch before anything was measured
    _sample_rows = staticmethod(sample_rows)              # (predict.py's native loop picks the same rows on the host)

    def _measure(self, eng: Engine, input_ids: torch.Tensor, first: bool) -> tuple[float, bool]:
        """One hearing of the mode in its current form: the seeded samples (`first`: they also place the short-read switch) and rows
        of this batch.  Returns the largest logit difference that counts against the mode (inf for anything non-finite) and whether
        the batch's own rows were measured in the mode (they are not when its reads take the fp16x3 kernels inside fp16c)."""
        B, L = input_ids.shape
        rep = self.selfcheck_report
        f16c = self.precision == "fp16c"
        worst = 0.0

        def measure(name, ids):
            diff, differ = eng.selfcheck(ids)
            rep.setdefault("samples", []).append({"sample": name, "max_abs_dlogit": diff, "labels_differ": differ,
                                                  "mlp_compensation": self._mlp_lo})
            return finite_or_inf(diff)

        if first:
            g = torch.Generator().manual_seed(20240)
            min_ok = None
            try:
                if f16c:
                    eng.set_f16c_min_len(1)                # measure the 16-bit kernels themselves at every sample length
                for Ls in self._SAMPLE_LENGTHS:
                    n = 4 if Ls >= 2048 else 8
                    ids = torch.randint(7, 11, (n, Ls), generator=g, dtype=torch.uint8)
                    ids[:, -1] = 1                          # [SEP]
                    ids[0, : Ls // 3] = 4                   # one read left-padded, as the collator pads
                    d = measure(f"synthetic {n} x {Ls}", ids.to(eng.device))
                    # LOWERING the switch below its unmeasured default rests on this one sample: it must pass with a margin of 2
                    # (round 4 lowered it to 512 on a sample at 4.7e-4 and the first real batch there sat at 94 % of the threshold)
                    if not d <= (self.selfcheck_tol if Ls >= self._DEFAULT_MIN_LEN else 0.5 * self.selfcheck_tol):
                        if not f16c:                        # fp16 / bf16 have no length switch: the sample IS the verdict
                            worst = max(worst, d)
                        break                               # fp16c: a failing sample moves the switch (below), it does not end the mode
                    worst = max(worst, d)
                    min_ok = Ls
                    if not f16c:
                        break                               # fp16 / bf16: one verdict, no length switch
            finally:
                # whatever happened in the loop (an engine error included) the handle never stays at "every length in 16 bits":
                # reads shorter than the shortest sample length that passed (with every longer one) take the fp16x3 kernels; if not
                # even the longest sample passed, everything up to its length does -- longer reads are judged by the rows of their
                # own batches (next lines; the error falls with the length)
                if f16c:
                    rep["f16c_min_len"] = min_ok if min_ok is not None else self._SAMPLE_LENGTHS[0] + 1
                    eng.set_f16c_min_len(rep["f16c_min_len"])
        measured = eng.effective_precision(L) == self.precision     # (fp16c: not for reads below the switch -- those run fp16x3)
        if measured:
            rows = self._sample_rows(B, self._BATCH_ROWS)
            sample = input_ids[rows] if rows != list(range(len(rows))) else input_ids[: len(rows)]
            worst = max(worst, measure(f"batch rows {rows} x {L}", sample))
        return worst, measured

    def _selfcheck(self, eng: Engine, input_ids: torch.Tensor) -> None:
        """See the class docstring; `guard` calls it where `guard_due` said so.  Runs on torch's current stream and synchronises it (a
        few ms per sample)."""
        L, rep, sched = input_ids.shape[1], self.selfcheck_report, self._guard
        first = not sched.heard
        worst, measured = self._measure(eng, input_ids, first)
        if not worst <= self.selfcheck_tol and self.precision == "fp16c" and not self._mlp_lo:
            # second level of the mode: fc1 / fc2 on hi + lo weights as well (their rounding shows on SOME weights: DESIGN.md
            # section 3) -- heard again from the start, samples included, before anybody falls back
            self._mlp_lo = True
            eng.set_mlp_compensation(True)
            rep["mlp_compensation"] = True
            logging.getLogger("chimeralm_amd").info(
                "chimeralm_amd: fp16c with plain-fp16 MLP weights measures %.2e on the loaded weights (threshold %.1e): "
                "switching the MLP to hi + lo weights (~10 %% slower) and measuring again", worst, self.selfcheck_tol)
            worst, measured = self._measure(eng, input_ids, True)
        rep.setdefault("mlp_compensation", False)
        rep["max_abs_dlogit"] = worst if first else max(rep.get("max_abs_dlogit", 0.0), worst)   # (of the form the mode is kept in)
        rep["tol"], rep["precision"] = self.selfcheck_tol, self.precision
        sched.record(L, worst, measured=measured)
        rep["checks"] = rep.get("checks", 0) + 1
        if not worst <= self.selfcheck_tol and not rep.get("fallback"):
            eng.set_fallback(1)
            announce_fallback(rep, subject="", precision=self.precision, worst=worst, tol=self.selfcheck_tol,
                              fallback_precision=eng.effective_precision(L))
        rep.setdefault("fallback", False)

    # The periodic re-check is meant to cost ~1 % of the work between two checks: two passes over 4 reads, one of them in exact fp32
    # (~19 read-equivalents).  At the bench's batch of 256 that is every 16th batch; at the reference's default batch of 12 sixteen
    # batches are 192 reads and the same rule costs 10 % -- so a periodic check also waits for this many READS since the last one
    # (round 5; 86 batches of 12).  The other triggers (first batch, length range, a measurement near the threshold) do not wait.
    selfcheck_min_reads = 1024

    def guard_due(self, n_tokens: int, n_reads: int | None = None) -> bool:
        """Is a self-check due for a batch of `n_tokens`-token reads (`GuardSchedule.due`)?  Never without `selfcheck`, in fp32 or once
        fallen back; fp16c's batches below the length switch are not on trial -- they take the fp16x3 kernels.  Counts the batch."""
        if not self.selfcheck or self.precision == "fp32" or self.selfcheck_report.get("fallback"):
            return False
        g = self._guard                                   # with this module's knobs as they are NOW: assignable after construction
        g.tol, g.every, g.min_reads = self.selfcheck_tol, self.selfcheck_every, self.selfcheck_min_reads
        return g.due(n_tokens, n_reads, on_trial=self.precision != "fp16c" or n_tokens >= self.selfcheck_report.get(
            "f16c_min_len", self._DEFAULT_MIN_LEN))

    def guard(self, eng: Engine, input_ids, n_tokens: int | None = None, n_reads: int | None = None) -> None:
        """Self-check of the 16-bit mode where one is due (`guard_due`).  `forward` calls it; loops that drive the engine directly
        (predict.run_predict_native) call it with a CALLABLE that returns the batch's ids on the device, so that nothing is
        copied for the batches -- almost all -- on which no check is due."""
        L = int(n_tokens if n_tokens is not None else input_ids.shape[1])
        if n_reads is None and not callable(input_ids):
            n_reads = int(input_ids.shape[0])
        if self.guard_due(L, n_reads):
            self._selfcheck(eng, input_ids() if callable(input_ids) else input_ids)

    def forward(self, input_ids: torch.Tensor, input_quals: torch.Tensor | None = None) -> torch.Tensor:
        """`input_quals` is accepted and ignored, exactly as the reference does (hyena.py:244-256).

        `freeze_backbone=True`, in training mode with autograd on: the logits carry a graph to the head's parameters (the fine-tune,
        headtrain.py: the backbone runs as in inference, the attention pooling forward and backward in the engine, the classifier in
        torch); `precision` must be "fp32" or "fp16x3".  `trainable=True` with an unfrozen backbone, in training mode with autograd on:
        the logits carry a graph to EVERY parameter (hyenatrain.py: the Hyena operator's core forward and backward in the engine,
        everything around it in torch; exact fp32).  Every other call is inference and returns logits without a graph -- also a
        module with an unfrozen backbone and without `trainable` in training mode, which is how a freshly built module is called
        everywhere: it does not train, and `ClassificationLit.training_step` says so."""
        if self.trainable and not self.freeze_backbone and self.training and torch.is_grad_enabled():
            from .hyenatrain import train_forward

            return train_forward(self, input_ids)
        if self.freeze_backbone and self.training and torch.is_grad_enabled():
            from .headtrain import check_train_precision, differentiable_logits

            check_train_precision(self.precision)             # (before anything touches a GPU)
            return differentiable_logits(self, input_ids)
        if input_ids.device.type != "cuda":
            raise RuntimeError("chimeralm_amd.HyenaDna runs on an MI355X only (move the batch to 'cuda'); "
                               "there is no CPU forward")
        eng = self.engine(input_ids.device)
        self.guard(eng, input_ids)
        req, traj = self.attention_request(), self.trajectory_request()
        if req is None and traj is None:
            return eng.forward(input_ids)
        logits, *extra = eng.forward(input_ids, attention=req, trajectory=traj)
        if traj is not None:
            self.last_trajectory = extra.pop()              # device tensors; nothing waits for them here
        if req is None:
            return logits
        att = extra[0]
        if self.attention_top_k is not None:
            self.last_attention = att                       # device tensors; nothing waits for them here
        if getattr(self.head, "save_attention", False):
            # the reference's contract (hyena.py:129-130, a CPU tensor [B, L, 1]): the kernel's weights of every chunk of the batch,
            # in the arithmetic the forward ran in, brought over by one D2H copy
            self.head.attention_weights = att.weights.cpu().unsqueeze(-1)
        return logits

    def micro_reads(self, n_tokens: int, device: torch.device) -> int:
        """Reads of `n_tokens` tokens the engine runs as one chunk (`clm_chunk_reads`): the micro-batch of the head fine-tune."""
        from .headtrain import train_engine

        return train_engine(self, torch.device(device)).chunk_reads_for(n_tokens)

    def trajectory_request(self):
        """The `engine.TrajectoryRequest` this module's forwards make (None: `trajectory_stride` is not set).  Loops that drive the
        engine directly pass it on themselves."""
        from .engine import TrajectoryRequest

        return None if self.trajectory_stride is None else TrajectoryRequest(stride=self.trajectory_stride, summary=True)

    def attention_request(self):
        """The `engine.AttentionRequest` this module's forwards make (None: none): peaks for `attention_top_k`, weights for
        `head.save_attention` or `attention_device_weights`.  Loops that drive the engine directly pass it on themselves."""
        from .engine import AttentionRequest

        weights = bool(getattr(self.head, "save_attention", False)) or (self.attention_top_k is not None and self.attention_device_weights)
        if self.attention_top_k is None and not weights:
            return None
        return AttentionRequest(top_k=self.attention_top_k, weights=weights)
