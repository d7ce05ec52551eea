"""`python eval.py ckpt_path=<ckpt|safetensors> +data.predict_data_path=<reads.bam> [data.batch_size=12] [hydra.run.dir=<out>]`
`python eval.py ckpt_path=<ckpt|safetensors> data=fq model=mambasp data.test_data_path=<reads.parquet>`

The Hydra entry route of the reference (/root/reference/eval.py:33-101, configs/eval.yaml): compose
configs/eval.yaml, instantiate datamodule / model / callbacks / trainer from their `_target_`s and run
`trainer.predict(model=model, dataloaders=datamodule, ckpt_path=cfg.ckpt_path, return_predictions=False)` when the data node has
a `predict_data_path`, `trainer.test(model=model, datamodule=datamodule, ckpt_path=cfg.ckpt_path)` otherwise (:74-80).
Prediction files land in `${paths.output_dir}/predicts/{rank}_{batch}.txt` (configs/callbacks/write.yaml); the test stage
leaves `test/loss`, `test/f1`, `test/precision`, `test/recall` in `trainer.callback_metrics` and logs them.
The built-in composer (chimeralm_amd/config.py) reads the files -- whether or not hydra-core is installed: one behaviour everywhere.
`+long_reads.mode=tile [+long_reads.overlap=4096] [+long_reads.max_bases=262144] [+long_reads.window=N]` on the predict route cuts reads
longer than the model's context into overlapping windows for whichever net `model=` names (chimeralm_amd/longread.py) and writes
`{rank}_{batch}.windows.tsv` next to the predictions; unknown keys are refused.
`+batching.mode=bucket [+batching.steps_log2=3]` on the predict route pads every read to a canonical length of its own and forwards reads
of one such length together (chimeralm_amd/bucket.py): a read's logits do not depend on its batch-mates; unknown keys are refused.
`+trajectory.stride=128 [+trajectory.values=true]` on the predict route also writes the running verdict of every read, from the same
forward, as `{rank}_{batch}.traj.tsv` (and `.traj.npz`) next to the predictions (chimeralm_amd/callbacks.py TrajectoryWriter), for the
causal nets (`model=` the Hyena net, mamba or mambasp); unknown keys are refused, and so is `+long_reads.mode=tile` with it.
Multi-GPU: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 eval.py trainer=ddp ...`.
"""
from __future__ import annotations

import logging
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

log = logging.getLogger("eval")


LONG_READ_KEYS = ("mode", "window", "overlap", "max_bases")


def long_read_options(cfg):
    """The `longread.Options` of `+long_reads.*` (None: no such node, or mode=truncate); unknown keys and bad values are a ValueError."""
    from chimeralm_amd.longread import Options

    node = dict(cfg.get("long_reads") or {})
    unknown = sorted(set(node) - set(LONG_READ_KEYS))
    if unknown:
        raise ValueError(f"unknown long_reads option(s) {unknown}; known: {list(LONG_READ_KEYS)}")
    if not node:
        return None
    options = Options(**{k: (str(v) if k == "mode" else v) for k, v in node.items()})     # a bad option fails before anything is loaded
    return options if options.mode == "tile" else None


BATCHING_KEYS = ("mode", "steps_log2")


def batching_options(cfg):
    """The `bucket.Options` of `+batching.*` (None: no such node, or mode=file); unknown keys and bad values are a ValueError."""
    from chimeralm_amd.bucket import Options

    node = dict(cfg.get("batching") or {})
    unknown = sorted(set(node) - set(BATCHING_KEYS))
    if unknown:
        raise ValueError(f"unknown batching option(s) {unknown}; known: {list(BATCHING_KEYS)}")
    if not node:
        return None
    options = Options(**{k: (str(v) if k == "mode" else v) for k, v in node.items()})     # a bad option fails before anything is loaded
    return options if options.mode == "bucket" else None


TRAJECTORY_KEYS = ("stride", "values")


def trajectory_options(cfg):
    """`(stride, values)` of `+trajectory.*` (None: no such node); unknown keys, a missing or bad stride and a `values` that is not a
    boolean are a ValueError."""
    from chimeralm_amd.engine import check_trajectory_stride

    node = dict(cfg.get("trajectory") or {})
    unknown = sorted(set(node) - set(TRAJECTORY_KEYS))
    if unknown:
        raise ValueError(f"unknown trajectory option(s) {unknown}; known: {list(TRAJECTORY_KEYS)}")
    if not node:
        return None
    stride, values = node.get("stride"), node.get("values", False)
    if isinstance(stride, bool) or not isinstance(stride, int):
        raise ValueError(f"+trajectory.stride must be an integer (a multiple of 128 in 128 ... 4096), got {stride!r}")
    if not isinstance(values, bool):
        raise ValueError(f"+trajectory.values must be true or false, got {values!r}")
    return check_trajectory_stride(stride), values                  # a bad option fails before anything is loaded


def _trajectory_writer(trajectory, model, trainer):
    """The net told its stride, and the `TrajectoryWriter` into the prediction writer's folder.  A net that has no such knob is left
    to the predict loop's refusal."""
    from chimeralm_amd.callbacks import TrajectoryWriter

    stride, values = trajectory
    if hasattr(model.net, "trajectory_request"):
        model.net.trajectory_stride = stride
    writers = [cb for cb in trainer.callbacks if hasattr(cb, "write_on_batch_end")]
    if not writers:
        raise ValueError("no prediction-writer callback configured (configs/callbacks/write.yaml)")
    return TrajectoryWriter(output_dir=writers[0].output_dir, values=values)


def evaluate(cfg):
    from chimeralm_amd.config import instantiate, instantiate_callbacks

    assert cfg.ckpt_path
    long_reads = long_read_options(cfg)
    batching = batching_options(cfg)
    trajectory = trajectory_options(cfg)
    if batching is not None and long_reads is not None:
        raise ValueError("+batching.mode=bucket and +long_reads.mode=tile exclude each other")
    if trajectory is not None and long_reads is not None:
        raise ValueError("+trajectory.stride and +long_reads.mode=tile exclude each other: a read reduced from several windows has no "
                         "single row to follow")
    log.info(f"Instantiating datamodule <{cfg.data._target_}>")
    datamodule = instantiate(cfg.data)
    log.info(f"Instantiating model <{cfg.model._target_}>")
    model = instantiate(cfg.model)
    log.info("Instantiating callbacks...")
    callbacks = instantiate_callbacks(cfg.get("callbacks"))
    log.info(f"Instantiating trainer <{cfg.trainer._target_}>")
    trainer = instantiate(cfg.trainer, callbacks=callbacks, logger=[])
    object_dict = {"cfg": cfg, "datamodule": datamodule, "model": model, "logger": [], "trainer": trainer}
    if getattr(datamodule, "predict_data_path", None) is None:
        if long_reads is not None:
            raise ValueError("+long_reads.mode=tile belongs to the predict route (+data.predict_data_path=<reads.bam>)")
        if batching is not None:
            raise ValueError("+batching.mode=bucket belongs to the predict route (+data.predict_data_path=<reads.bam>)")
        if trajectory is not None:
            raise ValueError("+trajectory.stride belongs to the predict route (+data.predict_data_path=<reads.bam>)")
        trainer.test(model=model, datamodule=datamodule, ckpt_path=cfg.ckpt_path)
    elif long_reads is not None:
        if not hasattr(datamodule, "max_length"):
            raise ValueError(f"+long_reads.mode=tile needs a datamodule that can deliver untruncated reads, not {cfg.data._target_}")
        datamodule.max_length = long_reads.max_tokens
        trainer.predict(model=model, dataloaders=datamodule, ckpt_path=cfg.ckpt_path, return_predictions=False, long_reads=long_reads)
    else:
        extra = {} if batching is None else {"batching": batching}
        if trajectory is not None:
            extra["trajectory_writer"] = _trajectory_writer(trajectory, model, trainer)
        trainer.predict(model=model, dataloaders=datamodule, ckpt_path=cfg.ckpt_path, return_predictions=False, **extra)
    return trainer.callback_metrics, object_dict


def main(argv: list[str] | None = None):
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    argv = list(sys.argv[1:] if argv is None else argv)
    # One composer everywhere: chimeralm_amd/config.py reads the same files and override grammar.  (`hydra.compose` outside
    # `@hydra.main` sets no HydraConfig, so configs/paths/default.yaml's ${hydra:runtime.output_dir} could not resolve, and
    # `hydra.run.dir=` would be taken as a plain override: an installed hydra-core would have crashed this route, not helped it.)
    from chimeralm_amd.config import compose

    out = next((a.split("=", 1)[1] for a in argv if a.startswith("hydra.run.dir=")), None)
    cfg = compose(ROOT / "configs", "eval.yaml", [a for a in argv if not a.startswith("hydra.")], output_dir=out)
    if cfg.get("extras", {}).get("print_config"):
        import yaml

        from chimeralm_amd.config import to_container

        log.info(yaml.safe_dump(to_container(cfg), sort_keys=False))
    return evaluate(cfg)


if __name__ == "__main__":
    main()
