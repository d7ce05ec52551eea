"""GPU (MI355X): the metric sums of the test stage (csrc/eval_metrics.hip through chimeralm_amd.eval_metrics.EvalMetrics) against
tests/golden/eval_golden.json -- torch.nn.CrossEntropyLoss in float64 and confusion counts by plain torch on the same fp32 logits.

Bounds: counts are integers and must be equal.  The kernel computes every row's loss in double from the same fp32 logits as the
fixture, so the two differ by the rounding of exp / log (a few ulp of 1.1e-16 per row) and by the order of a sum of at most a few
hundred positive terms: 1e-12 relative leaves three orders of magnitude over that."""
from __future__ import annotations

import json

import pytest
import torch

from eval_reference import COUNTS, host_result, result

pytestmark = pytest.mark.gpu
REL = 1e-12


@pytest.fixture(scope="module")
def cases(golden_dir):
    return json.loads((golden_dir / "eval_golden.json").read_text())["metrics"]


def _run(batches, ignore_index=-100, device="cuda:0"):
    from chimeralm_amd.eval_metrics import EvalMetrics

    dev = torch.device(device)
    m = EvalMetrics(dev, ignore_index=ignore_index)
    for logits, labels in batches:
        m.update(torch.as_tensor(logits, dtype=torch.float32).to(dev), torch.as_tensor(labels, dtype=torch.int64).to(dev))
    out = m.read()
    m.close()
    return out


def _close(got: float, want: float) -> bool:
    print(f"    got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    return abs(got - want) <= REL * abs(want)


def test_counts_and_losses_equal_the_fixture(cases, built_lib):
    from chimeralm_amd.eval_metrics import metrics_from_result

    assert [c["name"] for c in cases] == ["ignored", "one_class", "uneven"]
    for case in cases:
        print(case["name"])
        batches = [(b["logits"], b["labels"]) for b in case["batches"]]
        got = _run(batches, case["ignore_index"])
        for k, v in case["counts"].items():
            assert got[k] == v, (case["name"], k)
        assert got["n_batches"] == len(batches) and got["n_empty_batches"] == got["n_invalid_labels"] == got["n_nonfinite"] == 0
        assert got["tp"] + got["fp"] + got["tn"] + got["fn"] == got["n_valid"]
        m = metrics_from_result(got)
        assert _close(m["test/loss"], case["loss"]), case["name"]
        assert _close(m["test/loss_per_read"], case["loss_per_read"]), case["name"]
        assert _close(got["sum_loss"], sum(b["sum_loss"] for b in case["batches"])), case["name"]
        # every batch on its own is the fixture's batch (a fresh handle per batch)
        for b in case["batches"]:
            one = _run([(b["logits"], b["labels"])], case["ignore_index"])
            assert {k: one[k] for k in ("tp", "fp", "tn", "fn", "n_valid", "n_ignored")} == {
                k: b[k] for k in ("tp", "fp", "tn", "fn", "n_valid", "n_ignored")}
            assert abs(one["sum_batch_mean_loss"] - b["mean_loss"]) <= REL * abs(b["mean_loss"])
        # and the host statement of the same sums agrees on every field
        want = host_result(batches, case["ignore_index"])
        assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    one_class = metrics_from_result(_run([(b["logits"], b["labels"]) for b in cases[1]["batches"]]))
    assert one_class["test/tp"] + one_class["test/fp"] == 0
    assert (one_class["test/f1"], one_class["test/precision"], one_class["test/recall"]) == (0.0, 0.0, 0.0)


def test_two_runs_give_the_same_bits(cases, built_lib):
    for case in cases:
        batches = [(b["logits"], b["labels"]) for b in case["batches"]]
        a, b = _run(batches, case["ignore_index"]), _run(batches, case["ignore_index"])
        assert a == b, case["name"]
        assert a["sum_loss"].hex() == b["sum_loss"].hex() and a["sum_batch_mean_loss"].hex() == b["sum_batch_mean_loss"].hex()


def test_a_tie_predicts_class_zero(built_lib):
    got = _run([([[1.5, 1.5], [1.5, 1.5], [0.0, 1.0]], [1, 0, 1])])
    assert (got["tp"], got["fp"], got["tn"], got["fn"]) == (1, 0, 1, 1)


def test_bad_label_and_nan_logit_are_counted_not_summed(cases, built_lib):
    b = cases[2]["batches"][2]                                # 12 rows, none ignored
    logits, labels = [list(r) for r in b["logits"]], list(b["labels"])
    clean = _run([(logits, labels)])
    labels_bad = list(labels)
    labels_bad[3] = -1                                        # an id without "|label"
    labels_bad[7] = 2
    logits_bad = [list(r) for r in logits]
    logits_bad[5][1] = float("nan")
    logits_bad[9][0] = float("inf")
    logits_bad[3][0] = float("nan")                           # row 3 already has a bad label: counted once, as that
    got = _run([(logits_bad, labels_bad)])
    assert got["n_invalid_labels"] == 2 and got["n_nonfinite"] == 2 and got["n_valid"] == 8 and got["n_batches"] == 1
    keep = [i for i in range(12) if i not in (3, 5, 7, 9)]
    want = host_result([([logits[i] for i in keep], [labels[i] for i in keep])])
    assert {k: got[k] for k in ("tp", "fp", "tn", "fn", "n_valid")} == {k: want[k] for k in ("tp", "fp", "tn", "fn", "n_valid")}
    assert abs(got["sum_loss"] - want["sum_loss"]) <= REL * want["sum_loss"]
    assert got["sum_loss"] == got["sum_loss"] and got["sum_loss"] < clean["sum_loss"]         # finite, and smaller by four rows
    assert {k: got[k] for k in COUNTS} == {k: host_result([(logits_bad, labels_bad)])[k] for k in COUNTS}
    # a batch of nothing but such rows is an empty batch, and its rows are still counted
    got = _run([(logits, labels), ([[float("nan"), 0.0], [0.0, 0.0]], [1, 5])])
    assert got == {**clean, "n_empty_batches": 1, "n_invalid_labels": 1, "n_nonfinite": 1}


def test_a_batch_of_only_ignored_rows_changes_nothing_but_n_empty_batches(cases, built_lib):
    case = cases[0]
    batches = [(b["logits"], b["labels"]) for b in case["batches"]]
    ign = case["ignore_index"]
    base = _run(batches, ign)
    empty = ([[0.25, -1.0]] * 5, [ign] * 5)
    for where in (0, 1, len(batches)):
        got = _run(batches[:where] + [empty] + batches[where:], ign)
        assert got == {**base, "n_empty_batches": 1}, where
    assert _run([empty, empty], ign) == result(n_empty_batches=2)


def test_reset_merge_and_argument_checks(cases, built_lib):
    from chimeralm_amd.eval_metrics import EvalError, EvalMetrics, merge_results

    dev = torch.device("cuda:0")
    batches = [(torch.tensor(b["logits"], dtype=torch.float32, device=dev), torch.tensor(b["labels"], device=dev))
               for b in cases[2]["batches"]]
    m = EvalMetrics(dev)
    for lg, lb in batches[:2]:
        m.update(lg, lb)
    first = m.read()
    m.reset()
    assert m.read() == result()
    for lg, lb in batches[2:]:
        m.update(lg, lb)
    second = m.read()
    m.merge(first)                                            # another rank's sums on top of this handle's
    both = m.read()
    whole = _run([(b["logits"], b["labels"]) for b in cases[2]["batches"]])
    assert {k: both[k] for k in COUNTS} == {k: whole[k] for k in COUNTS}
    assert both["sum_loss"] == second["sum_loss"] + first["sum_loss"]
    assert merge_results([first, second])["sum_loss"] == first["sum_loss"] + second["sum_loss"]
    # a strided view is made contiguous, a wrong dtype / shape / device is refused
    wide = torch.zeros((12, 4), dtype=torch.float32, device=dev)
    wide[:, :2] = batches[2][0]
    m.reset()
    m.update(wide[:, :2], batches[2][1])
    assert m.read() == _run([(cases[2]["batches"][2]["logits"], cases[2]["batches"][2]["labels"])])
    for lg, lb in ((batches[0][0].double(), batches[0][1]), (batches[0][0], batches[0][1].int()), (batches[0][0].cpu(), batches[0][1]),
                   (batches[1][0], batches[0][1]), (torch.zeros((4, 3), device=dev), torch.zeros(4, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError):
            m.update(lg, lb)
    m.close()
    with pytest.raises(EvalError, match="n_classes"):
        EvalMetrics(dev, n_classes=3)
