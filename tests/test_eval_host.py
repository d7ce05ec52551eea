"""The test stage without a GPU: the metric formulas, merging results through the library's host-only handle, the C ABI
exports, and the module / trainer checks that run before the first batch."""
from __future__ import annotations

import ctypes
import json
import re
from pathlib import Path

import pytest
import torch

from eval_reference import COUNTS, host_result, result as _result

REPO = Path(__file__).resolve().parent.parent


def test_metric_formulas_and_zero_denominators():
    from chimeralm_amd.eval_metrics import metrics_from_result

    m = metrics_from_result(_result(tp=6, fp=2, tn=9, fn=3, n_valid=20, n_batches=2, sum_batch_mean_loss=1.5, sum_loss=12.0))
    assert m["test/precision"] == 6 / 8 and m["test/recall"] == 6 / 9 and m["test/f1"] == 12 / 17
    assert m["test/loss"] == 0.75 and m["test/loss_per_read"] == 0.6
    assert m["test/tp"] == 6 and m["test/n_valid"] == 20 and m["test/n_invalid_labels"] == 0
    # f1 is the harmonic mean of the two
    p, r = m["test/precision"], m["test/recall"]
    assert abs(m["test/f1"] - 2 * p * r / (p + r)) < 1e-15
    # class 1 never predicted: precision has no denominator -> 0; recall and f1 are plain zeros
    m = metrics_from_result(_result(tn=5, fn=4, n_valid=9, n_batches=1, sum_batch_mean_loss=0.3, sum_loss=2.7))
    assert (m["test/precision"], m["test/recall"], m["test/f1"]) == (0.0, 0.0, 0.0)
    # no positive read: recall has no denominator -> 0
    m = metrics_from_result(_result(fp=2, tn=5, n_valid=7, n_batches=1))
    assert (m["test/precision"], m["test/recall"], m["test/f1"]) == (0.0, 0.0, 0.0)
    # nothing predicted positive and nothing positive: all three denominators are 0, and so are loss's with no batch at all
    m = metrics_from_result(_result(tn=3, n_valid=3, n_batches=1, sum_batch_mean_loss=0.1, sum_loss=0.3))
    assert (m["test/precision"], m["test/recall"], m["test/f1"]) == (0.0, 0.0, 0.0)
    m = metrics_from_result(_result())
    assert all(m[k] == 0.0 for k in ("test/loss", "test/loss_per_read", "test/f1", "test/precision", "test/recall"))
    assert all(isinstance(m[k], float) for k in ("test/loss", "test/f1", "test/precision", "test/recall", "test/loss_per_read"))


def test_merge_of_two_results_equals_the_concatenated_batches(built_lib, golden_dir):
    from chimeralm_amd.eval_metrics import EvalError, EvalMetrics, merge_results

    gold = json.loads((golden_dir / "eval_golden.json").read_text())["metrics"]
    for case in gold:
        batches = [(b["logits"], b["labels"]) for b in case["batches"]]
        cut = len(batches) // 2 + 1
        a, b, whole = host_result(batches[:cut]), host_result(batches[cut:]), host_result(batches)
        merged = merge_results([a, b])
        for k in COUNTS:
            assert merged[k] == whole[k], (case["name"], k)
        assert {k: whole[k] for k in ("tp", "fp", "tn", "fn", "n_valid", "n_ignored")} == case["counts"]
        assert abs(merged["sum_loss"] - whole["sum_loss"]) <= 1e-12 * whole["sum_loss"]
        assert abs(merged["sum_batch_mean_loss"] - whole["sum_batch_mean_loss"]) <= 1e-12 * whole["sum_batch_mean_loss"]
        assert merged["sum_loss"] == a["sum_loss"] + b["sum_loss"]           # one addition per rank, in list order
        # the host statement of the sums is the fixture's torch.nn.CrossEntropyLoss
        assert abs(whole["sum_batch_mean_loss"] / whole["n_batches"] - case["loss"]) <= 1e-12 * case["loss"]
        assert abs(whole["sum_loss"] / whole["n_valid"] - case["loss_per_read"]) <= 1e-12 * case["loss_per_read"]
    # the host-only handle totals and resets; it cannot take a batch
    h = EvalMetrics(None)
    h.merge(_result(tp=1, n_valid=1, n_batches=1, sum_loss=0.25, sum_batch_mean_loss=0.25))
    h.merge(_result(fn=2, n_valid=2, n_batches=1, n_invalid_labels=3, sum_loss=0.5, sum_batch_mean_loss=0.25))
    assert h.read() == _result(tp=1, fn=2, n_valid=3, n_batches=2, n_invalid_labels=3, sum_loss=0.75, sum_batch_mean_loss=0.5)
    h.reset()
    assert h.read() == _result()
    h.close()
    with pytest.raises(EvalError, match="n_classes must be 2"):
        EvalMetrics(None, n_classes=3)
    with pytest.raises(EvalError, match="ignore_index"):
        EvalMetrics(None, ignore_index=1)


def test_eval_abi_is_exported(built_lib):
    from chimeralm_amd import _native

    lib = ctypes.CDLL(str(built_lib))
    hdr = (REPO / "include" / "chimeralm_hip.h").read_text()
    names = ("clm_eval_create", "clm_eval_update", "clm_eval_read", "clm_eval_merge", "clm_eval_reset", "clm_eval_last_error",
             "clm_eval_destroy")
    for name in names:
        assert hasattr(lib, name) and name in _native.SYMBOLS and f"{name}(" in hdr
    assert set(names) == {n for n in _native.SYMBOLS if n.startswith("clm_eval_")} == set(re.findall(r"\b(clm_eval_[a-z_]+)\s*\(", hdr))
    assert lib.clm_abi_version() == _native.ABI_VERSION == 6 and "#define CLM_ABI_VERSION 6" in hdr
    # the binding's struct is the header's: ten int64 counts, then two doubles
    assert ctypes.sizeof(_native.ClmEvalResult) == 96
    fields = re.search(r"typedef struct clm_eval_result \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)[,;]", fields) == [f[0] for f in _native.ClmEvalResult._fields_]
    lib2 = _native.load()
    h = ctypes.c_void_p()
    assert lib2.clm_eval_create(-1, 2, -100, ctypes.byref(h)) == 0
    assert lib2.clm_eval_update(h, None, None, 4, None) == _native.E_STATE and b"host-only" in lib2.clm_eval_last_error(h)
    assert lib2.clm_eval_read(h, None, None) == _native.E_INVALID and lib2.clm_eval_merge(h, None) == _native.E_INVALID
    assert lib2.clm_eval_destroy(h) == 0 and lib2.clm_eval_destroy(None) == 0


def test_eval_kernel_has_no_scratch(built_lib):
    from chimeralm_amd import build as B

    txt = B.RESOURCES.read_text()
    blocks = [b for b in txt.split("Function Name: ") if b.startswith("_ZN3clm4eval18eval_update_kernel")]
    assert len(blocks) == 1
    assert "ScratchSize [bytes/lane]: 0" in blocks[0]


def test_module_steps_and_criterion_check():
    from chimeralm_amd.basic_module import ClassificationLit

    class Net(torch.nn.Module):
        number_of_classes = 2

        def forward(self, input_ids, input_quals=None):
            return torch.stack([input_ids.float().mean(1), -input_ids.float().mean(1) + 9.0], dim=1)

    model = ClassificationLit(Net())
    assert type(model.criterion) is torch.nn.CrossEntropyLoss and model.test_criterion() == -100
    assert list(model.state_dict()) == []                      # the default criterion adds nothing to a checkpoint's keys
    batch = {"input_ids": torch.tensor([[7, 8, 9, 10], [1, 1, 1, 1]]), "labels": torch.tensor([0, 1])}
    loss, preds, targets = model.model_step(batch)
    logits, labels = model.predict_step(batch, 0)
    assert preds.tolist() == [0, 1] and targets is batch["labels"] and labels is batch["labels"]
    assert abs(float(loss) - float(torch.nn.functional.cross_entropy(logits, labels))) < 1e-7
    with pytest.raises(RuntimeError, match="Trainer.test attaches"):
        model.test_step(batch, 0)
    assert ClassificationLit(Net(), criterion=torch.nn.CrossEntropyLoss(ignore_index=-1)).test_criterion() == -1
    for bad in (torch.nn.BCEWithLogitsLoss(), torch.nn.CrossEntropyLoss(label_smoothing=0.1),
                torch.nn.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0])), torch.nn.CrossEntropyLoss(reduction="sum")):
        with pytest.raises(NotImplementedError, match="CrossEntropyLoss"):
            ClassificationLit(Net(), criterion=bad).test_criterion()


def test_trainer_test_refuses_before_the_first_batch(golden_dir):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.trainer import Trainer

    class Net(torch.nn.Module):
        number_of_classes = 2

    class Loader:
        def test_dataloader(self):
            raise AssertionError("the data must not be touched")

        def setup(self, *a, **k):
            raise AssertionError("the data must not be touched")

    t = Trainer()
    with pytest.raises(NotImplementedError, match="CrossEntropyLoss"):
        t.test(ClassificationLit(Net(), criterion=torch.nn.NLLLoss()), datamodule=Loader())
    with pytest.raises(ValueError, match="test_dataloader"):
        t.test(ClassificationLit(Net()), datamodule=object())
    assert t.callback_metrics == {}
