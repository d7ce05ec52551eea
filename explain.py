"""`python explain.py ckpt_path=<ckpt|safetensors> model=mambasp +data.predict_data_path=<reads.bam> [+explain.window=3]
[+explain.stride=2] [+explain.substitute=N|all] [+explain.score=prob|gap] [+explain.top_k=10] [+explain.values=true]
[+explain.max_reads=N] [+explain.batch_size=256] [hydra.run.dir=<out>]`

In-silico mutagenesis for any `model=` (hyena, transformer, cnn, mamba, mambasp): which bases of each read the prediction rests on.
The reference has the analysis for one read on the host (chimeralm/explain/motif.py:64-82, `get_position_importance`) and no entry
point for it; this one composes configs/eval.yaml with the composer `eval.py` uses, instantiates datamodule, model and trainer from
their `_target_`s and runs `trainer.explain(...)`.  Results land in `${paths.output_dir}/explain/{rank}_explain.tsv` (and
`{rank}_{index}.explain.npz` with `+explain.values=true`).
"""
from __future__ import annotations

import logging
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

log = logging.getLogger("explain")
OPTION_KEYS = ("window", "stride", "substitute", "score", "top_k")


def explain(cfg):
    from chimeralm_amd.callbacks import ExplainWriter
    from chimeralm_amd.config import instantiate
    from chimeralm_amd.explain import Options

    assert cfg.ckpt_path
    node = dict(cfg.get("explain") or {})
    unknown = sorted(set(node) - set(OPTION_KEYS) - {"values", "max_reads", "batch_size"})
    if unknown:
        raise ValueError(f"unknown explain option(s) {unknown}")
    options = {k: node[k] for k in OPTION_KEYS if k in node}
    if "substitute" in options:
        options["substitute"] = str(options["substitute"])
    Options(**options)                                        # a bad option fails before anything is loaded
    log.info(f"Instantiating datamodule <{cfg.data._target_}>")
    datamodule = instantiate(cfg.data)
    if getattr(datamodule, "predict_data_path", None) is None:
        raise ValueError("explain.py scans the reads of +data.predict_data_path=<reads.bam>")
    log.info(f"Instantiating model <{cfg.model._target_}>")
    model = instantiate(cfg.model)
    log.info(f"Instantiating trainer <{cfg.trainer._target_}>")
    trainer = instantiate(cfg.trainer, callbacks=[], logger=[])
    writer = ExplainWriter(Path(cfg.paths.output_dir) / "explain", values=bool(node.get("values", False)))
    n = trainer.explain(model=model, datamodule=datamodule, ckpt_path=cfg.ckpt_path, writer=writer, max_reads=node.get("max_reads"),
                        batch_size=int(node.get("batch_size", 256)), **options)
    return n, {"cfg": cfg, "datamodule": datamodule, "model": model, "trainer": trainer, "writer": writer}


def main(argv: list[str] | None = None):
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    argv = list(sys.argv[1:] if argv is None else argv)
    from chimeralm_amd.config import compose

    out = next((a.split("=", 1)[1] for a in argv if a.startswith("hydra.run.dir=")), None)
    cfg = compose(ROOT / "configs", "eval.yaml", [a for a in argv if not a.startswith("hydra.")], output_dir=out)
    return explain(cfg)


if __name__ == "__main__":
    main()
