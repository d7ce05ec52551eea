"""The decisions the nets share about their 16-bit arithmetic, in plain Python (imports neither torch nor the engine library): WHEN a
mode is measured again against exact fp32 and what is said when it fails (`HyenaDna`, `SequenceCNNTransformer`), and whether the
loaded weights fit fp16x3's packing (all four).  The nets keep which samples they measure and how they call their engine."""
from __future__ import annotations

import logging
import warnings

from ._native import X3_WEIGHT_LIMIT

_LOG = logging.getLogger("chimeralm_amd")


class GuardSchedule:
    """Which batches a guarded mode is measured on since the last weight load.  `tol`, `every` and `min_reads` are plain attributes:
    the owning net copies its own knobs (`selfcheck_tol`, `selfcheck_every`, `selfcheck_min_reads`) into them in its `guard_due`,
    where every hearing starts, so that assigning those after construction keeps working."""

    def __init__(self, tol: float, every: int, min_reads: int = 0):
        self.tol, self.every, self.min_reads = tol, every, min_reads
        self.reset()

    def reset(self) -> None:
        """New weights: the mode gets a new hearing."""
        self.heard = False                                        # a hearing was recorded since the last weight load
        self.checked_min_len = self.checked_max_len = None        # shortest / longest batch MEASURED in the mode since then ...
        self.batches_since_check = self.reads_since_check = 0     # ... and what went by since the last check
        self.recheck_next = False                                 # the last measurement was kept within 10 % of the threshold

    def due(self, n_tokens: int, n_reads: int | None = None, *, on_trial: bool = True) -> bool:
        """Is a check due for a batch of `n_tokens`-token reads?  The first batch since a weight load; then, for batches that run in
        the mode (`on_trial`; the others are neither measured nor counted): the first such batch, a batch whose length leaves the range
        already measured by more than a factor 1.5 in EITHER direction (the error is neither monotone in the length nor the same from
        batch to batch: profiles/r03_fp16c_margin.txt), the batch after a measurement within 10 % of the threshold, and every
        `every`-th batch once `min_reads` reads went by as well (`n_reads` unknown: not waited for).  Counts the batch."""
        if not self.heard:
            return True
        if not on_trial:
            return False
        if self.checked_min_len is None:
            return True
        self.batches_since_check += 1
        self.reads_since_check += int(n_reads) if n_reads is not None else self.min_reads
        return (self.recheck_next or 3 * n_tokens < 2 * self.checked_min_len or 2 * n_tokens > 3 * self.checked_max_len
                or (self.every > 0 and self.batches_since_check >= self.every and self.reads_since_check >= self.min_reads))

    def record(self, n_tokens: int, worst: float, *, measured: bool = True) -> None:
        """A hearing on a batch of `n_tokens`-token reads gave `worst` (`finite_or_inf`).  Only a batch that really ran in the mode
        (`measured`) widens the checked range.  Kept, but within 10 % of the threshold: the spread from batch to batch at
        fixed weights is 2-3x (profiles/r04_fp16c_margin.txt), so the NEXT batch is measured too instead of the `every`-th from now."""
        self.heard = True
        if measured:
            self.checked_min_len = n_tokens if self.checked_min_len is None else min(n_tokens, self.checked_min_len)
            self.checked_max_len = max(n_tokens, self.checked_max_len or 0)
        self.batches_since_check = self.reads_since_check = 0
        self.recheck_next = measured and 0.9 * self.tol < worst <= self.tol


def sample_rows(B: int, n: int) -> list[int]:
    """`n` rows spread evenly over a batch of B (not its first rows: a file sorted by anything would make those alike)."""
    return list(range(B)) if B <= n else sorted({round(i * (B - 1) / (n - 1)) for i in range(n)})


def finite_or_inf(x: float) -> float:
    """A measured difference as the verdicts compare it: NaN counts as inf."""
    return x if x == x else float("inf")


def announce_fallback(report: dict, *, subject: str, precision: str, worst: float, tol: float, fallback_precision: str) -> None:
    """The mode fell back for good: into the report, the log and a RuntimeWarning pointing at the caller's caller of the net's method."""
    report["fallback"] = True
    report["fallback_precision"] = fallback_precision
    what = ("exact fp32 (the reference's arithmetic)" if fallback_precision == "fp32" else
            "fp16x3 (every operand as two halfs, three fp16 MFMAs per product: fp32-class logits, about half the rate)")
    msg = (f"chimeralm_amd: {subject}precision={precision!r} differs from the exact-fp32 kernels by {worst:.2e} in the logits on the "
           f"loaded weights (threshold {tol:.1e}); falling back to {what} for this model")
    _LOG.warning(msg)
    warnings.warn(msg, RuntimeWarning, stacklevel=4)


def x3_range_report(subject: str, precision: str, weights, *, effective: str | None = None, where: str = "",
                    tail: str = "this model runs the exact-fp32 kernels") -> dict:
    """`precision_report` of the weights just loaded.  fp16x3 packs weights x 2^10 as fp16 halfs, which saturate at |w| >=
    X3_WEIGHT_LIMIT: such weights run the exact-fp32 kernels wherever the mode would run fp16x3, and one warning says so.
    `weights`: the tensors that are packed (looked at only when `precision` is not fp32).  `effective`: what the engine reads back
    for the place this mode uses fp16x3 -- its verdict; None: the verdict is taken here, on the largest weight (a NaN maximum falls back).
    `where` / `tail`: the subject's own words for that place and for what happens instead."""
    if precision == "fp32":
        return {"precision": "fp32", "fallback": False}
    wmax = max(float(w.detach().abs().max()) for w in weights)
    fallback = not wmax < X3_WEIGHT_LIMIT if effective is None else effective != "fp16x3"
    report = {"precision": precision, "max_abs_weight": wmax, "fallback": fallback}
    if fallback:
        report["fallback_precision"] = effective or "fp32"
        _LOG.warning(f"chimeralm_amd: {subject} precision={precision!r} packs weights as fp16 halfs x 2^10{where}, which saturate at "
                     f"|w| >= {X3_WEIGHT_LIMIT:g}; the loaded weights reach {wmax:.3g}, so {tail}")
    return report
