"""Prediction files, mirroring /root/reference/chimeralm/models/callbacks.py.

`resume_read_name` (:38-63) and `PredictionWriter.write_on_batch_end` (:79-150): one file
`{output_dir}/{global_rank}_{batch_idx}.txt` per batch, one line `name<TAB>label` per read, label = argmax of logits.

Difference kept on purpose: the id row is decoded with its length byte read as UNSIGNED, so read names of
128..255 characters work; the reference's collator raises on them (torch.tensor(..., dtype=int8) overflow,
tokenizer.py:168), so no input the reference accepts is treated differently.

`AttentionWriter` has no counterpart there: the reference keeps `attention_weights` of ONE forward on the module (hyena.py:129-130)
and notebooks/attention.ipynb works from that; here the engine's per-read summary and peaks (csrc/attn_weights.hip) are written
per batch next to the predictions, under names `filter` does not glob (`*.txt`, filter.py).

`ExplainWriter` writes what the mutagenesis scan (explain.py, csrc/explain.hip) found per read; the reference's counterpart
(chimeralm/explain/motif.py) plots one read's scores and writes no file.

`WindowWriter` writes the per-window table of `predict --long-reads tile` (longread.py, csrc/longread.hip); the reference truncates
a long read and has nothing to write.

`TrajectoryWriter` writes the running verdict of `predict --save-trajectory` (csrc/trajectory.hip): after how many bases the model's
label settles and where the evidence arrives; the reference has no counterpart.
"""
from __future__ import annotations

import io
import logging
import zipfile
from pathlib import Path
from typing import Any

import numpy as np
import torch

log = logging.getLogger(__name__)


def resume_read_name(bytes_data) -> str:
    if isinstance(bytes_data, torch.Tensor):
        if bytes_data.numel() == 0:
            return ""
        bytes_data = bytes_data.tolist()
    elif bytes_data is None or len(bytes_data) == 0:
        return ""
    data = [int(b) & 0xFF for b in bytes_data]
    n = data[0]
    if n <= 0 or n >= len(data):
        raise ValueError("Invalid read name data")
    return "".join(chr(b) for b in data[1: 1 + n] if 32 <= b <= 126)


class PredictionWriter:
    """Same constructor and hook signature as the reference (a Lightning BasePredictionWriter there)."""

    def __init__(self, output_dir: str | Path, write_interval: str = "batch") -> None:
        self.output_dir = Path(output_dir)
        self.interval = write_interval

    def write_on_batch_end(self, trainer: Any, pl_module: Any, prediction: Any, batch_indices: Any,
                           batch: dict[str, Any], batch_idx: int, dataloader_idx: int = 0) -> None:
        if prediction is None or "id" not in batch:
            log.error("batch %d: missing prediction or 'id'", batch_idx)
            return
        pred = prediction[0] if isinstance(prediction, (list, tuple)) else prediction
        if pred is None or pred.numel() == 0:
            log.warning("Empty prediction tensor for batch %d", batch_idx)
            return
        labels = pred.argmax(dim=1).cpu().tolist()     # device boundary: D2H + sync, as in the reference (:107)
        ids = batch["id"].cpu() if isinstance(batch["id"], torch.Tensor) else batch["id"]
        if len(labels) != len(ids):
            log.error("Size mismatch: predictions=%d, batch_ids=%d for batch %d", len(labels), len(ids), batch_idx)
            return
        lines = []
        for i, row in enumerate(ids):
            try:
                name = resume_read_name(row) or f"unknown_read_{i}"
            except ValueError:
                name = f"error_read_{i}"
            lines.append(f"{name}\t{labels[i]}\n")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        with (self.output_dir / f"{rank}_{batch_idx}.txt").open("w") as f:
            f.writelines(lines)


def _read_names(ids) -> list[str]:
    """Names of a batch's id rows, with `PredictionWriter`'s fall-backs."""
    names = []
    for i, row in enumerate(ids):
        try:
            names.append(resume_read_name(row) or f"unknown_read_{i}")
        except ValueError:
            names.append(f"error_read_{i}")
    return names


def _npz_bytes(arrays: dict[str, np.ndarray]) -> bytes:
    """An uncompressed `.npz` (np.load reads it) whose bytes depend on the arrays alone: np.savez stamps its members with the time."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as zf:
        for name, arr in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arr), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


class AttentionWriter:
    """Where in each read the model looked: one `{rank}_{batch_idx}.attn.tsv` per batch, one line per read,

        name<TAB>label<TAB>n_bases<TAB>n_pad<TAB>pad_weight<TAB>sep_weight<TAB>pos:weight;pos:weight;...

    with the read's largest-weight bases in descending weight (`pos` 0-based among the read's bases, weights as %.6g; an empty
    field for a read without bases), and with `weights=True` one `{rank}_{batch_idx}.attn.npz` holding `names`, `n_bases` int32
    [B], `offsets` int64 [B + 1] and `weights` fp32: the per-base weights of all reads concatenated, [PAD] and [SEP] stripped
    (read i: weights[offsets[i]:offsets[i + 1]]).  `attention` is an `engine.AttentionOutput` of HOST tensors."""

    def __init__(self, output_dir: str | Path, weights: bool = False) -> None:
        self.output_dir = Path(output_dir)
        self.weights = bool(weights)

    def write_on_batch_end(self, trainer: Any, pl_module: Any, prediction: Any, attention: Any, batch: dict[str, Any],
                           batch_idx: int) -> None:
        if prediction is None or attention is None or attention.summary is None or "id" not in batch:
            log.error("batch %d: missing prediction, attention summary or 'id'", batch_idx)
            return
        pred = prediction[0] if isinstance(prediction, (list, tuple)) else prediction
        labels = pred.argmax(dim=1).tolist()
        ids = batch["id"].cpu() if isinstance(batch["id"], torch.Tensor) else batch["id"]
        f = {k: v.tolist() for k, v in attention.fields().items()}
        if not len(labels) == len(ids) == len(f["n_bases"]):
            log.error("Size mismatch: predictions=%d, batch_ids=%d, attention=%d for batch %d", len(labels), len(ids),
                      len(f["n_bases"]), batch_idx)
            return
        names = _read_names(ids)
        pos, wgt = attention.peak_pos.tolist(), attention.peak_weight.tolist()
        lines = []
        for i, name in enumerate(names):
            n = f["n_peaks"][i]
            peaks = ";".join(f"{p}:{w:.6g}" for p, w in zip(pos[i][:n], wgt[i][:n]))
            lines.append(f"{name}\t{labels[i]}\t{f['n_bases'][i]}\t{f['n_pad'][i]}\t{f['pad_weight'][i]:.6g}\t"
                         f"{f['sep_weight'][i]:.6g}\t{peaks}\n")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        with (self.output_dir / f"{rank}_{batch_idx}.attn.tsv").open("w") as fh:
            fh.writelines(lines)
        if not self.weights:
            return
        if attention.weights is None:
            log.error("batch %d: per-base weights were asked for but the forward left none", batch_idx)
            return
        w = attention.weights.numpy()
        n_bases = np.asarray(f["n_bases"], dtype=np.int32)
        offsets = np.zeros(len(names) + 1, dtype=np.int64)
        np.cumsum(n_bases, out=offsets[1:])
        flat = np.concatenate([w[i, p: p + n] for i, (p, n) in enumerate(zip(f["n_pad"], f["n_bases"]))] or [np.zeros(0, np.float32)])
        (self.output_dir / f"{rank}_{batch_idx}.attn.npz").write_bytes(_npz_bytes(
            {"names": np.asarray(names, dtype=np.str_), "n_bases": n_bases, "offsets": offsets, "weights": flat.astype(np.float32)}))


class ExplainWriter:
    """Which bases a read's prediction rests on (explain.position_importance): one `{rank}_explain.tsv` per rank, one line per read,

        name<TAB>label<TAB>p1<TAB>logit0<TAB>logit1<TAB>n_bases<TAB>window<TAB>stride<TAB>substitute<TAB>score<TAB>pos:value;...<TAB>n_nonfinite

    with label, p1 = softmax(logits)[1] (in double) and the logits of the unmodified read, the scan's options, and the read's bases
    of largest importance in descending order (`pos` 0-based among the read's bases, numbers as %.6g; an empty field for a read that
    reports no peaks).  With `values=True` also one `{rank}_{index}.explain.npz` per read (`index` counts this rank's reads) holding
    `name` [1], `logits`, `dp1`, `dgap`, `importance`, `peak_pos`, `peak_val` and `n_nonfinite`.  `importance` is an `explain.Importance`
    of HOST tensors.  The file of a rank starts empty with the writer's first read.  `filter`'s `*.txt` glob sees neither name."""

    def __init__(self, output_dir: str | Path, values: bool = False) -> None:
        self.output_dir = Path(output_dir)
        self.values = bool(values)
        self._started: set = set()

    @staticmethod
    def line(name: str, importance: Any) -> str:
        lg = importance.logits[0].tolist()
        l0, l1 = float(lg[0]), float(lg[1])
        label = int(l1 > l0)                                    # a tie is class 0, as torch.argmax
        p1 = float("nan")
        if np.isfinite(l0) and np.isfinite(l1):
            e0, e1 = np.exp(np.float64(l0) - max(l0, l1)), np.exp(np.float64(l1) - max(l0, l1))
            p1 = float(e1 / (e0 + e1))
        o = importance.options
        pos, val = importance.peak_pos.tolist(), importance.peak_val.tolist()
        peaks = ";".join(f"{p}:{v:.6g}" for p, v in zip(pos, val) if p >= 0)
        return (f"{name}\t{label}\t{p1:.6g}\t{l0:.7g}\t{l1:.7g}\t{importance.n_bases}\t{o.window}\t{o.stride}\t{o.substitute}\t"
                f"{o.score}\t{peaks}\t{int(importance.n_nonfinite[0])}\n")

    def write_read(self, trainer: Any, name: str, index: int, importance: Any) -> None:
        self.output_dir.mkdir(parents=True, exist_ok=True)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        path = self.output_dir / f"{rank}_explain.tsv"
        with path.open("a" if path in self._started else "w") as fh:
            fh.write(self.line(name, importance))
        self._started.add(path)
        if self.values:
            arrays = {"name": np.asarray([name], dtype=np.str_)}
            arrays.update({k: v.numpy() for k, v in importance.tensors().items()})
            (self.output_dir / f"{rank}_{index}.explain.npz").write_bytes(_npz_bytes(arrays))


class WindowWriter:
    """Which window of a long read decided its label (longread.tiled_forward): one `{rank}_{batch_idx}.windows.tsv` per batch that
    holds a read of more than one window, one line per such read,

        name<TAB>n_bases<TAB>n_windows<TAB>chosen<TAB>start:end:logit0:logit1;...<TAB>n_nonfinite

    with the bases looked at (after the cap), the chosen window's index, every window's bases [start, end) among the read's and its
    logits (%.7g) in window order, and the number of windows with a non-finite logit.  The read's line in `{rank}_{batch_idx}.txt`
    carries the chosen window's label.  `tiled` is a `longread.TiledLogits` of HOST tensors.  A batch without a long read writes no
    file; `filter`'s `*.txt` glob does not see the name."""

    def __init__(self, output_dir: str | Path) -> None:
        self.output_dir = Path(output_dir)

    def write_on_batch_end(self, trainer: Any, tiled: Any, batch: dict[str, Any], batch_idx: int) -> None:
        if tiled is None or tiled.plan.n_extra == 0:
            return
        if tiled.chosen is None or "id" not in batch:
            log.error("batch %d: missing window table or 'id'", batch_idx)
            return
        plan = tiled.plan
        ids = batch["id"].cpu() if isinstance(batch["id"], torch.Tensor) else batch["id"]
        if len(ids) != plan.B:
            log.error("Size mismatch: windows of %d reads, batch_ids=%d for batch %d", plan.B, len(ids), batch_idx)
            return
        names = _read_names(ids)
        wl, chosen, bad = tiled.window_logits.tolist(), tiled.chosen.tolist(), tiled.nonfinite.tolist()
        wb = plan.C - 1
        lines = []
        for r in range(plan.B):
            win = plan.windows_of(r)
            if len(win) < 2:
                continue
            table = ";".join(f"{s}:{s + wb}:{wl[i][0]:.7g}:{wl[i][1]:.7g}" for i, s in win)
            lines.append(f"{names[r]}\t{int(plan.n_bases[r])}\t{len(win)}\t{chosen[r]}\t{table}\t{bad[r]}\n")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        with (self.output_dir / f"{rank}_{batch_idx}.windows.tsv").open("w") as fh:
            fh.writelines(lines)


class TrajectoryWriter:
    """After how many bases the model decides (engine.TrajectoryOutput, csrc/trajectory.hip): one `{rank}_{batch_idx}.traj.tsv` per
    batch, one line per read,

        name<TAB>label<TAB>n_bases<TAB>K<TAB>first<TAB>onset<TAB>before_jump<TAB>at_jump<TAB>jump_dgap<TAB>final_gap

    with the label of the whole row (the sign of logit1 - logit0, a tie is 0), the number of points K, and as BASES SEEN -- the read's
    bases inside the point, clamp(n_k - n_pad, 0, n_bases) -- the first point that holds a base, the point from which the label no
    longer changes (onset_k), and the two points either side of the largest step of the gap towards the label (jump_k - 1, jump_k)
    with that step and the final gap as %.7g; a point that does not exist (a non-finite curve, a read of one informative point) is
    -1.  With `values=True` also one `{rank}_{batch_idx}.traj.npz` holding `names`, `traj` fp32 [B, K, 2] (logits at every point)
    and `bases_seen` int32 [B, K].  `trajectory` is an `engine.TrajectoryOutput` of HOST tensors with a summary.  `filter`'s `*.txt`
    glob sees neither name."""

    def __init__(self, output_dir: str | Path, values: bool = False) -> None:
        self.output_dir = Path(output_dir)
        self.values = bool(values)

    def write_on_batch_end(self, trainer: Any, trajectory: Any, batch: dict[str, Any], batch_idx: int) -> None:
        if trajectory is None or trajectory.summary is None or "id" not in batch:
            log.error("batch %d: missing trajectory summary or 'id'", batch_idx)
            return
        ids = batch["id"].cpu() if isinstance(batch["id"], torch.Tensor) else batch["id"]
        f = {k: v.tolist() for k, v in trajectory.fields().items()}
        if len(ids) != len(f["label"]):
            log.error("Size mismatch: trajectories of %d reads, batch_ids=%d for batch %d", len(f["label"]), len(ids), batch_idx)
            return
        names = _read_names(ids)
        seen = trajectory.bases_seen()

        def at(i: int, k: int) -> int:
            return int(seen[i, k]) if k >= 0 else -1

        lines = []
        for i, name in enumerate(names):
            jump = f["jump_k"][i]
            lines.append(f"{name}\t{f['label'][i]}\t{f['n_bases'][i]}\t{f['n_points'][i]}\t{at(i, f['first_k'][i])}\t{at(i, f['onset_k'][i])}\t"
                         f"{at(i, jump - 1 if jump >= 0 else -1)}\t{at(i, jump)}\t{f['jump_dgap'][i]:.7g}\t{f['final_gap'][i]:.7g}\n")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        with (self.output_dir / f"{rank}_{batch_idx}.traj.tsv").open("w") as fh:
            fh.writelines(lines)
        if self.values:
            (self.output_dir / f"{rank}_{batch_idx}.traj.npz").write_bytes(_npz_bytes(
                {"names": np.asarray(names, dtype=np.str_), "traj": trajectory.logits.numpy(), "bases_seen": seen}))
