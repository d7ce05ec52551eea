"""One rank of `python eval.py <overrides>` for tests/test_gpu_test_stage.py, with two taps the product route does not have: every
batch the metrics kernel was given (logits and labels, cloned on the device, copied back after the stage) goes to
`<out>/rank<r>.pt`, and `trainer.callback_metrics` to `<out>/metrics<r>.json`.  Not a test module.

    python tests/eval_stage_driver.py <out dir> <eval.py overrides ...>
    python -m torch.distributed.run --nproc-per-node 2 ... tests/eval_stage_driver.py <out dir> <eval.py overrides ...>
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def main():
    out, overrides = Path(sys.argv[1]), sys.argv[2:]
    import torch

    from chimeralm_amd.eval_metrics import EvalMetrics

    seen = []
    update = EvalMetrics.update

    def tapped(self, logits, labels):
        seen.append((logits.clone(), labels.clone()))
        return update(self, logits, labels)

    EvalMetrics.update = tapped
    spec = importlib.util.spec_from_file_location("eval_entry", REPO / "eval.py")
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    metrics, objects = entry.main(overrides)
    rank = int(os.environ.get("RANK", 0))
    out.mkdir(parents=True, exist_ok=True)
    torch.save([(lg.cpu(), lb.cpu()) for lg, lb in seen], out / f"rank{rank}.pt")
    (out / f"metrics{rank}.json").write_text(json.dumps(metrics))
    assert metrics is objects["trainer"].callback_metrics


if __name__ == "__main__":
    main()
