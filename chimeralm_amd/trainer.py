"""`Trainer` for the predict and test stages: what `lightning.pytorch.trainer.Trainer` does for the reference's
`trainer.predict(model=model, dataloaders=datamodule, ckpt_path=cfg.ckpt_path, return_predictions=False)`
(/root/reference/eval.py:74-80; configs/trainer/{default,gpu,ddp}.yaml for the constructor keywords), without Lightning:
one process per GPU (torchrun environment), the datamodule set up for this rank, the MI355X predict loop
(`chimeralm_amd.predict.run_predict`), the prediction-writer callbacks.  `test` is `trainer.test(model=model, datamodule=datamodule,
ckpt_path=cfg.ckpt_path)` of the same file: the test loop (`run_test`) with the metric sums kept on the device, one read of them at
the end, one all-gather of that small struct across ranks, and the reference's metric names in `callback_metrics`.  Training keywords
(`min_epochs`, `max_epochs`, `check_val_every_n_epoch`, ...) are accepted and ignored: this class has no `fit`; the engine's five
training paths -- the Hyena head on a frozen backbone, DNAConvNet, the two Mamba nets, SequenceCNNTransformer and the whole HyenaDna
net -- are the `fit_*` functions over `chimeralm_amd.fit.fit` (`python -m chimeralm_amd finetune` / `train`).
`explain` has no Lightning counterpart: the predict datamodule's reads through the mutagenesis scan (`run_explain`), for any net.
"""
from __future__ import annotations

import logging
import os
from pathlib import Path

import torch

from . import distributed
from .predict import run_explain, run_predict, run_test

log = logging.getLogger(__name__)


class Trainer:
    def __init__(self, accelerator: str = "gpu", devices: int | str = 1, callbacks: list | None = None, logger=None,
                 default_root_dir: str | None = None, deterministic: bool = False, strategy: str | None = None,
                 num_nodes: int = 1, **training_only):
        if accelerator not in ("gpu", "cuda", "auto"):
            raise ValueError(f"accelerator={accelerator!r}: this engine runs on MI355X GPUs only (no CPU path exists)")
        if num_nodes != 1:
            raise ValueError("one node (up to 8 GPUs over xGMI) is what the predict path shards over")
        self.devices, self.callbacks, self.logger = devices, list(callbacks or []), logger
        self.default_root_dir, self.deterministic, self.strategy = default_root_dir, deterministic, strategy
        self.callback_metrics: dict = {}
        self.global_rank, self.local_rank, self.world_size = distributed.env_world()

    def _start(self) -> tuple[int, int, torch.device]:
        """Join the process group (torchrun environment) and make this rank's GPU current.  CLM_DIST_BACKEND=gloo with
        CLM_RANKS_SHARE_GPU=1 is the one-GPU rehearsal of a multi-GPU run, as in `python -m chimeralm_amd predict`."""
        rank, local_rank, world = distributed.init_process_group(os.environ.get("CLM_DIST_BACKEND"))
        self.global_rank, self.local_rank, self.world_size = rank, local_rank, world
        if self.devices not in (-1, "auto") and int(self.devices) != world:
            log.warning("trainer.devices=%s but WORLD_SIZE=%d: one process per GPU is launched by torchrun "
                        "(python -m torch.distributed.run --nproc-per-node N eval.py ...)", self.devices, world)
        share = os.environ.get("CLM_RANKS_SHARE_GPU") == "1"
        device = torch.device("cuda", local_rank % torch.cuda.device_count() if share else local_rank)
        torch.cuda.set_device(device)
        return rank, world, device

    def predict(self, model, dataloaders=None, datamodule=None, ckpt_path: str | Path | None = None,
                return_predictions: bool = False, *, long_reads=None, batching=None, trajectory_writer=None):
        """`long_reads` (a `longread.Options` of mode "tile"): reads longer than the window are judged in overlapping windows, for
        any net; the datamodule must deliver them untruncated (`max_length=long_reads.max_tokens`).  `batching` (a `bucket.Options`
        of mode "bucket"): every read is padded to a canonical length of its own and reads of one such length are forwarded
        together, for any net; each rank regroups its own shard.  `trajectory_writer` (a `callbacks.TrajectoryWriter`): the running
        verdict of every batch is written too, for a causal net built with `trajectory_stride`."""
        dm = datamodule if datamodule is not None else dataloaders
        if dm is None or not hasattr(dm, "predict_dataloader"):
            raise ValueError("Trainer.predict needs a datamodule with predict_dataloader()")
        rank, world, device = self._start()
        if ckpt_path is not None:
            log.info("Loading checkpoint %s", ckpt_path)
            model.load_reference_checkpoint(ckpt_path)
        dm.setup("predict", world_size=world, rank=rank)
        writers = [cb for cb in self.callbacks if hasattr(cb, "write_on_batch_end")]
        if not writers:
            raise ValueError("no prediction-writer callback configured (configs/callbacks/write.yaml)")
        n = run_predict(model, dm, writers[0], device, rank=rank, long_reads=long_reads, batching=batching,
                        trajectory_writer=trajectory_writer)
        distributed.barrier()
        log.info("[rank %d] %d reads predicted", rank, n)
        return None

    def explain(self, model, datamodule=None, dataloaders=None, ckpt_path: str | Path | None = None, *, writer=None,
                max_reads: int | None = None, batch_size: int = 256, **options) -> int:
        """Per-base importance of the predict datamodule's reads under `model` (any net), written by `writer` (a
        callbacks.ExplainWriter); `options` are explain.position_importance's.  Each rank scans the reads of its shard.  Returns the
        number of reads this rank wrote."""
        dm = datamodule if datamodule is not None else dataloaders
        if dm is None or not hasattr(dm, "predict_dataloader"):
            raise ValueError("Trainer.explain needs a datamodule with predict_dataloader()")
        if writer is None or not hasattr(writer, "write_read"):
            raise ValueError("Trainer.explain needs a writer with write_read() (callbacks.ExplainWriter)")
        rank, world, device = self._start()
        if ckpt_path is not None:
            log.info("Loading checkpoint %s", ckpt_path)
            model.load_reference_checkpoint(ckpt_path)
        dm.setup("predict", world_size=world, rank=rank)
        n = run_explain(model, dm, writer, device, rank=rank, max_reads=max_reads, batch_size=batch_size, **options)
        distributed.barrier()
        log.info("[rank %d] %d reads scanned", rank, n)
        return n

    def test(self, model, datamodule=None, dataloaders=None, ckpt_path: str | Path | None = None) -> list[dict]:
        """Loss, F1, precision and recall of `model` over the datamodule's labelled test set, as `lightning.Trainer.test` reports
        them for the reference's `test_step`: a list of one dict, also left in `callback_metrics`.  Every rank returns the same
        numbers.  Raises, instead of reporting over part of the data, if a label was neither 0, 1 nor the criterion's
        `ignore_index`, or a logit was not finite."""
        from .eval_metrics import EvalMetrics, merge_results, metrics_from_result, result_from_dict, result_to_dict
        from . import _native as N

        dm = datamodule if datamodule is not None else dataloaders
        if dm is None or not hasattr(dm, "test_dataloader"):
            raise ValueError("Trainer.test needs a datamodule with test_dataloader() (data=fq)")
        ignore_index = model.test_criterion()                 # before the first batch: the kernel implements that one loss
        rank, world, device = self._start()
        if ckpt_path is not None:
            log.info("Loading checkpoint %s", ckpt_path)
            model.load_reference_checkpoint(ckpt_path)
        dm.setup("test", world_size=world, rank=rank)
        metrics = EvalMetrics(device, n_classes=model.net.number_of_classes, ignore_index=ignore_index)
        model.test_metrics = metrics
        try:
            n = run_test(model, dm, device)
            mine = metrics.read()                             # the one wait of the stage
        finally:
            model.test_metrics = None
            metrics.close()
        log.info("[rank %d] %d reads tested", rank, n)
        results = [mine]
        if world > 1:
            raw = torch.frombuffer(bytearray(bytes(result_from_dict(mine))), dtype=torch.uint8)
            if torch.distributed.get_backend() == "nccl":
                raw = raw.to(device)
            parts = [torch.empty_like(raw) for _ in range(world)]
            torch.distributed.all_gather(parts, raw)
            results = [result_to_dict(N.ClmEvalResult.from_buffer_copy(p.cpu().numpy().tobytes())) for p in parts]
        total = merge_results(results, ignore_index)          # rank order on every rank: the same bits everywhere
        if total["n_invalid_labels"] or total["n_nonfinite"]:
            raise RuntimeError(f"test stage: {total['n_invalid_labels']} reads carry a label that is neither 0, 1 nor ignore_index "
                               f"({ignore_index}) -- an id without '|<label>' parses to -1 -- and {total['n_nonfinite']} reads got a "
                               f"non-finite logit; no metrics are reported over part of the data")
        out = metrics_from_result(total)
        self.callback_metrics = dict(out)
        if rank == 0:
            width = max(len(k) for k in out)
            rows = [f"  {k:<{width}}  {v:.10g}" if isinstance(v, float) else f"  {k:<{width}}  {v}" for k, v in out.items()]
            log.info("Test metrics (%d reads, %d ranks)\n%s", total["n_valid"], world, "\n".join(rows))
        return [out]
