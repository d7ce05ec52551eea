"""CPU: chimeralm_amd/_guard.py on its own -- the schedule of the self-checks rule by rule, the row choice, the fall-back announcement
and the fp16x3 weight-range report.  No net and no engine; the schedule tests need no torch either (the module imports none).  The
expected message texts are the ones recorded before the code moved here (tests/golden/guard_traces.json, tests/test_guard_traces.py)."""
from __future__ import annotations

import json
import logging
import subprocess
import sys
import warnings
from pathlib import Path

import pytest

from chimeralm_amd._guard import GuardSchedule, announce_fallback, finite_or_inf, sample_rows, x3_range_report

GOLDEN = json.loads((Path(__file__).parent / "golden" / "guard_traces.json").read_text())
TOL = 5e-4


def _heard(every=16, min_reads=0, L=3000, worst=1e-4) -> GuardSchedule:
    g = GuardSchedule(TOL, every, min_reads)
    g.record(L, worst)
    return g


def _state(g):
    return (g.heard, g.checked_min_len, g.checked_max_len, g.batches_since_check, g.reads_since_check, g.recheck_next)


def test_the_module_imports_neither_torch_nor_the_engine_library():
    code = "import sys, chimeralm_amd._guard; assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules)"
    assert subprocess.run([sys.executable, "-c", code], cwd=Path(__file__).parent.parent).returncode == 0


def test_nothing_heard_yet_is_due_whatever_the_batch_and_counts_nothing():
    g = GuardSchedule(TOL, 16, 1024)
    assert _state(g) == (False, None, None, 0, 0, False)
    assert g.due(3000) and g.due(10, 5, on_trial=False)                           # (the seeded samples do not depend on the batch)
    assert _state(g) == (False, None, None, 0, 0, False)


def test_a_batch_that_is_not_on_trial_is_not_due_and_changes_no_counter():
    g = _heard(every=2)
    before = _state(g)
    for _ in range(5):
        assert not g.due(100, 12, on_trial=False)                                 # (far outside the window, past `every`: still nothing)
    assert _state(g) == before
    g2 = GuardSchedule(TOL, 2)
    g2.record(3000, 1e-4, measured=False)                                         # heard, but nothing measured in the mode yet
    assert not g2.due(3000, on_trial=False) and _state(g2)[3:5] == (0, 0)
    assert g2.due(3000) and _state(g2)[3:5] == (0, 0)                             # the first batch that runs the mode: due, not counted


def test_the_length_window_is_a_factor_of_one_and_a_half_in_either_direction():
    g = _heard(every=0)
    assert [g.due(L) for L in (3000, 2000, 4500)] == [False] * 3                  # 2/3 and 3/2 of the checked length are inside
    assert g.due(1999) and g.due(4501)
    g.record(1999, 1e-4), g.record(4501, 1e-4)
    assert (g.checked_min_len, g.checked_max_len) == (1999, 4501)
    assert [g.due(L) for L in (1333, 6751, 3000)] == [False] * 3 and g.due(1332) and g.due(6752)


def test_every_nth_batch_once_enough_reads_went_by():
    g = _heard(every=3)
    assert [g.due(3000) for _ in range(3)] == [False, False, True]
    assert [g.due(3000) for _ in range(2)] == [True, True]                        # stays due until a check is recorded
    g.record(3000, 1e-4)
    assert (g.batches_since_check, g.reads_since_check) == (0, 0) and not g.due(3000)
    g = _heard(every=2, min_reads=30)
    assert [g.due(3000, 12) for _ in range(3)] == [False, False, True]            # 2 batches are 24 reads: the third makes 36
    g.record(3000, 1e-4)
    assert [g.due(3000) for _ in range(2)] == [False, True]                       # batch size unknown: counted as `min_reads`
    g = _heard(every=0)
    assert not any(g.due(3000, 10**6) for _ in range(100))                        # every = 0: no periodic check


def test_a_measurement_kept_within_ten_percent_of_the_threshold_rearms_the_next_batch():
    for worst, rearm in ((0.9 * TOL, False), (0.96 * TOL, True), (TOL, True), (1.01 * TOL, False), (float("inf"), False), (0.0, False)):
        g = _heard(worst=worst)
        assert g.recheck_next is rearm and g.due(3000) is rearm
    g = _heard(worst=0.96 * TOL)
    g.record(3000, 1e-4)
    assert g.recheck_next is False and not g.due(3000)                            # released by the next reading


def test_a_hearing_that_measured_nothing_in_the_mode_leaves_the_range_and_clears_the_rearm():
    g = _heard(worst=0.96 * TOL)
    g.due(3000, 7)
    g.record(100, 0.96 * TOL, measured=False)
    assert _state(g) == (True, 3000, 3000, 0, 0, False)
    g = GuardSchedule(TOL, 16)
    g.record(100, 0.0, measured=False)
    assert _state(g) == (True, None, None, 0, 0, False)


def test_reset_is_a_weight_load_and_the_knobs_are_plain_attributes():
    g = _heard(every=3, worst=0.96 * TOL)
    g.due(3000, 5)
    g.reset()
    assert _state(g) == (False, None, None, 0, 0, False) and (g.tol, g.every, g.min_reads) == (TOL, 3, 0)
    g.record(3000, 1e-4)
    g.every = 1                                                                   # (the nets copy their knobs in before every question)
    assert g.due(3000)


def test_rows_are_spread_over_the_batch_and_nan_counts_as_inf():
    assert [sample_rows(B, 4) for B in (1, 4, 5, 40)] == [[0], [0, 1, 2, 3], [0, 1, 3, 4], [0, 13, 26, 39]]
    assert finite_or_inf(float("nan")) == float("inf") == finite_or_inf(float("inf")) and finite_or_inf(3e-4) == 3e-4


def _outer(report, **kw):
    def guard_method():
        def net_method():
            announce_fallback(report, **kw)
        net_method()
    guard_method()                                                                # <- the warning points here: the caller of the guard


@pytest.mark.parametrize("scenario, subject", [("hy_fp16x3_falls_back_to_fp32", ""), ("hy_both_levels_fail", ""),
                                               ("tf_drift_fp16x3_to_fp32", "SequenceCNNTransformer "),
                                               ("tf_drift_fp16c_to_fp16x3", "SequenceCNNTransformer ")])
def test_the_fallback_announcement_is_the_recorded_text(scenario, subject, caplog):
    want, rep = GOLDEN[scenario]["warnings"][0][0], GOLDEN[scenario]["selfcheck_report"][0]
    report: dict = {}
    with caplog.at_level(logging.WARNING, logger="chimeralm_amd"), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _outer(report, subject=subject, precision=rep["precision"], worst=rep["max_abs_dlogit"], tol=rep["tol"],
               fallback_precision=rep["fallback_precision"])
    assert report == {"fallback": True, "fallback_precision": rep["fallback_precision"]}
    assert [str(w.message) for w in caught] == [want] == [r.getMessage() for r in caplog.records]
    assert caught[0].category is RuntimeWarning and caught[0].filename == __file__
    assert caught[0].lineno == _outer.__code__.co_firstlineno + 5


# ----------------------------------------------------------------------------------------------- x3_range_report
_SUBJECT = {   # scenario prefix -> the arguments the net passes (chimeralm_amd/{hyena,transformer,cnn,mamba}.py)
    "x3_hyena_fp16c": dict(subject="HyenaDna", precision="fp16c", engine=True, tail="it runs the exact-fp32 kernels there",
                           where=" for fp16x3 (its reads below f16c_min_len and its first fall-back level)"),
    "x3_transformer_fp16x3": dict(subject="SequenceCNNTransformer", precision="fp16x3", engine=True, where=" for fp16x3",
                                  tail="it runs the exact-fp32 kernels there"),
    "x3_cnn": dict(subject="DNAConvNet", precision="fp16x3", engine=False),
    "x3_mamba": dict(subject="MambaSequenceClassification", precision="fp16x3", engine=False),
}


@pytest.mark.parametrize("value", ["63.9", "64", "nan"])
@pytest.mark.parametrize("prefix", sorted(_SUBJECT))
def test_the_weight_range_report_is_the_recorded_one(prefix, value, caplog):
    import torch

    want = GOLDEN[f"{prefix}_{value}"]
    kw = dict(_SUBJECT[prefix])
    ws = [torch.full((3, 2), -float(value)), torch.full((4,), 0.5)]
    if kw.pop("engine"):                                                          # the engine's read-back is the verdict
        kw["effective"] = "fp16x3" if abs(float(value)) < 64 else "fp32"
    with caplog.at_level(logging.WARNING, logger="chimeralm_amd"):
        rep = x3_range_report(kw.pop("subject"), kw.pop("precision"), iter(ws), **kw)
    nan = value == "nan"
    assert {k: v for k, v in rep.items() if not (nan and k == "max_abs_weight")} == {
        k: v for k, v in want["precision_report"][0].items() if not (nan and k == "max_abs_weight")}
    assert not nan or rep["max_abs_weight"] != rep["max_abs_weight"]
    assert [[r.levelname, r.getMessage()] for r in caplog.records] == want["logs"]
    assert rep["fallback"] is (value != "63.9") and len(want["logs"]) == int(rep["fallback"])


def test_fp32_needs_no_weights_and_an_engine_verdict_overrules_the_range(caplog):
    import torch

    for prefix in ("x3_hyena", "x3_transformer", "x3_cnn", "x3_mamba"):
        assert x3_range_report("X", "fp32", iter(())) == GOLDEN[f"{prefix}_fp32"]["precision_report"][0] == {"precision": "fp32", "fallback": False}
    with caplog.at_level(logging.WARNING, logger="chimeralm_amd"):
        assert x3_range_report("X", "fp16c", [torch.full((2,), 100.0)], effective="fp16x3") == {
            "precision": "fp16c", "max_abs_weight": 100.0, "fallback": False}
        assert caplog.records == []
        assert x3_range_report("X", "fp16c", [torch.full((2,), 1.0)], effective="fp32")["fallback_precision"] == "fp32"
        assert len(caplog.records) == 1
