"""The sums of the test stage (csrc/eval_metrics.hip) stated on the host with plain torch in float64: what the GPU tests and the
merge test compare against.  Not a test module."""
from __future__ import annotations

import torch

COUNTS = ("tp", "fp", "tn", "fn", "n_valid", "n_ignored", "n_batches", "n_empty_batches", "n_invalid_labels", "n_nonfinite")


def result(**kw):
    return {**{k: 0 for k in COUNTS}, "sum_batch_mean_loss": 0.0, "sum_loss": 0.0, **kw}


def host_result(batches, ignore_index=-100) -> dict:
    """What the kernel is specified to sum, by plain torch in float64 on the host, batch by batch."""
    r = result()
    for logits, labels in batches:
        logits, labels = torch.as_tensor(logits, dtype=torch.float32), torch.as_tensor(labels, dtype=torch.int64)
        keep = labels != ignore_index
        bad_label = keep & (labels != 0) & (labels != 1)
        nonfinite = keep & ~bad_label & ~torch.isfinite(logits).all(dim=1)
        valid = keep & ~bad_label & ~nonfinite
        r["n_invalid_labels"] += int(bad_label.sum())
        r["n_nonfinite"] += int(nonfinite.sum())
        if not valid.any():
            r["n_empty_batches"] += 1
            continue
        lg, lb = logits[valid].double(), labels[valid]
        pred = torch.argmax(lg.float(), dim=-1)
        loss = float(torch.nn.functional.cross_entropy(lg, lb, reduction="sum"))
        r["tp"] += int(((pred == 1) & (lb == 1)).sum())
        r["fp"] += int(((pred == 1) & (lb == 0)).sum())
        r["tn"] += int(((pred == 0) & (lb == 0)).sum())
        r["fn"] += int(((pred == 0) & (lb == 1)).sum())
        r["n_valid"] += int(valid.sum())
        r["n_ignored"] += int((~keep).sum())
        r["n_batches"] += 1
        r["sum_batch_mean_loss"] += loss / int(valid.sum())
        r["sum_loss"] += loss
    return r
