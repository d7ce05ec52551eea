"""`ClassificationLit` for the predict and test paths, mirroring /root/reference/chimeralm/models/basic_module.py.

Same constructor (`net, optimizer, scheduler, criterion, *, compile`), `forward(input_ids, input_quals)` (:67-77),
`predict_step(batch, batch_idx) -> (logits, labels)` (:177-187), `model_step(batch) -> (loss, preds, targets)` (:87-104) and
`test_step(batch, batch_idx)` (:153-170).  The reference's `test_step` feeds torchmetrics objects on the host; here it queues the
batch's sums on the device (eval_metrics.EvalMetrics, attached by `Trainer.test`).  When `lightning` is importable the class is a
`LightningModule`; otherwise a plain `nn.Module`.  Of the reference's training hooks `training_step` exists, for the five paths this
engine can differentiate: the Hyena head on a frozen backbone (headtrain.py) and, end to end, DNAConvNet (cnntrain.py), the two Mamba
nets (mambatrain.py), SequenceCNNTransformer (tftrain.py) and the whole HyenaDna net (hyenatrain.py); the Lightning hooks around it
(`on_train_start`, `configure_optimizers`, the epoch-end logging) are out of scope: `fit.fit` is the loop, under each module's `fit_*`.
"""
from __future__ import annotations

from typing import Any

import torch
from torch import nn

try:  # optional: not installed in the build image
    from lightning import LightningModule as _Base
except ImportError:  # pragma: no cover - depends on the environment
    _Base = nn.Module


class ClassificationLit(_Base):
    def __init__(self, net: nn.Module, optimizer: Any = None, scheduler: Any = None, criterion: nn.Module | None = None,
                 *, compile: bool = False):  # noqa: A002 - reference keyword
        super().__init__()
        if not hasattr(net, "number_of_classes"):
            raise AttributeError("net must expose `number_of_classes` (basic_module.py:43-58)")
        self.net = net
        # configs/model/*.yaml carry no `criterion` node: the loss of the reference's model files is the default
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()
        self.test_metrics = None                                # eval_metrics.EvalMetrics while Trainer.test runs
        self.optimizer_factory, self.scheduler_factory, self.compile_flag = optimizer, scheduler, compile

    def forward(self, input_ids: torch.Tensor, input_quals: torch.Tensor | None = None) -> torch.Tensor:
        return self.net(input_ids, input_quals)

    def predict_step(self, batch: dict[str, torch.Tensor], batch_idx: int = 0):
        logits = self.forward(batch["input_ids"], batch.get("input_quals", None))
        return logits, batch["labels"]

    def model_step(self, batch: dict[str, torch.Tensor]):
        """(loss, preds, targets) of one batch, as the reference computes them: torch ops on the logits' device, for callers that
        want one batch's numbers.  The test stage does not come through here (`test_step`)."""
        logits = self.forward(batch["input_ids"], batch.get("input_quals", None))
        targets = batch["labels"].to(logits.device)
        loss = self.criterion(logits.reshape(-1, logits.size(-1)), targets.long().view(-1))
        return loss, torch.argmax(logits, dim=-1), targets

    def training_step(self, batch: dict[str, torch.Tensor], batch_idx: int = 0) -> torch.Tensor:
        """The batch's loss with a graph to the trained parameters (basic_module.py `training_step`): for a net built with
        `freeze_backbone=True` (HyenaDna: the head's) or `trainable=True` (DNAConvNet, the Mamba nets, SequenceCNNTransformer, HyenaDna
        with an unfrozen backbone: all of them), in training mode.  No other backward exists on this engine; the error's wording
        dates from when only the head trained and is matched by tests."""
        if not getattr(self.net, "freeze_backbone", False) and not getattr(self.net, "trainable", False):
            raise NotImplementedError("only the head trains on this engine: freeze_backbone=True")
        loss, _, _ = self.model_step(batch)
        if not loss.requires_grad:
            raise RuntimeError("training_step: the loss has no graph -- the module is in eval() or autograd is off (model.train(), no no_grad)")
        return loss

    def test_step(self, batch: dict[str, torch.Tensor], batch_idx: int = 0) -> None:
        """Forward, then the batch's loss and confusion counts added to `self.test_metrics` by one kernel on the same stream."""
        if self.test_metrics is None:
            raise RuntimeError("test_step needs `test_metrics` (an eval_metrics.EvalMetrics); Trainer.test attaches one")
        logits = self.forward(batch["input_ids"], batch.get("input_quals", None))
        self.test_metrics.update(logits, batch["labels"].to(logits.device, non_blocking=True))

    def test_criterion(self) -> int:
        """`ignore_index` of the criterion, if it is the loss the metrics kernel implements; raises otherwise."""
        c = self.criterion
        if type(c) is not nn.CrossEntropyLoss or c.weight is not None or c.label_smoothing != 0.0 or c.reduction != "mean":
            raise NotImplementedError(f"the test stage implements torch.nn.CrossEntropyLoss (no class weights, no label smoothing, "
                                      f"mean reduction), not {c!r}")
        return int(c.ignore_index)

    # ---- checkpoint loading (reference: PyTorchModelHubMixin.from_pretrained / Lightning ckpt_path) ----
    def load_reference_checkpoint(self, path) -> "ClassificationLit":
        """Load `model.safetensors` (HF hub layout of `yangliz5/chimeralm`) or a Lightning `.ckpt`."""
        path = str(path)
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file

            sd = load_file(path)
        else:
            # a Lightning .ckpt is a pickle: load tensors only.  Checkpoints that also pickle arbitrary objects (hyper-parameter
            # partials, callbacks) need the full unpickler, which executes code from the file -- opt in explicitly.
            import os
            import pickle

            try:
                obj = torch.load(path, map_location="cpu", weights_only=True)
            except (pickle.UnpicklingError, RuntimeError) as e:
                if os.environ.get("CLM_TRUST_CHECKPOINT") != "1":
                    raise RuntimeError(
                        f"{path} holds pickled Python objects besides tensors; loading it would run code from the file. "
                        "Re-run with CLM_TRUST_CHECKPOINT=1 if you trust its origin, or convert it to safetensors.") from e
                obj = torch.load(path, map_location="cpu", weights_only=False)
            sd = obj.get("state_dict", obj)
        own = self.state_dict()
        # safetensors drops the aliases of the shared sine module; restore them from `.1.freq`
        for k in list(own):
            if k not in sd and (".implicit_filter.3.freq" in k or ".implicit_filter.5.freq" in k):
                src = k.replace(".3.freq", ".1.freq").replace(".5.freq", ".1.freq")
                if src in sd:
                    sd[k] = sd[src]
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"checkpoint lacks {len(missing)} tensors, e.g. {missing[:3]}")
        self.load_state_dict({k: sd[k] for k in own}, strict=True)
        return self
