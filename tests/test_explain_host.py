"""Host side of the mutagenesis scan (chimeralm_amd/explain.py, csrc/explain.hip's clm_explain_plan, callbacks.ExplainWriter): no GPU.

The plan builder is held to a brute-force enumeration written from the definition in include/chimeralm_hip.h."""
import ctypes
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from explain_reference import brute_force_plan, make_read as _read, mutant_rows

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n_bases,w,s", [(1, 1, 1), (65, 1, 1), (65, 3, 2), (131, 5, 3), (200, 5, 5)])
def test_plan_matches_brute_force(built_lib, n_bases, w, s):
    from chimeralm_amd import explain as E

    ids = _read(n_bases, 100 + n_bases)
    plan, n_windows = E.build_plan(ids, w, s, "N")
    want, want_windows = brute_force_plan(ids, w, s, "N")
    assert n_windows == want_windows == -(-n_bases // s)
    assert [(int(p["start"]), int(p["sub"]), int(p["slot"])) for p in plan] == want
    assert not plan["reserved"].any()
    # every base is covered by a window; the last window is clipped at the last base
    rows = mutant_rows(ids, want, w)
    assert (rows[:, -1] == 1).all() and ((rows[:, :-1] == 11).sum(0) >= 1).all()
    assert (rows[:, :-1] == 11).sum(1).max() <= w


def test_plan_all_on_a_read_with_n(built_lib):
    from chimeralm_amd import explain as E

    ids = _read(67, 7, with_n=True)
    n_is_n = int((ids[:-1] == 11).sum())
    assert n_is_n >= 1
    plan, n_windows = E.build_plan(ids, 1, 1, "all")
    want, _ = brute_force_plan(ids, 1, 1, "all")
    assert n_windows == 67 and len(plan) == 3 * (67 - n_is_n) + 4 * n_is_n
    assert [(int(p["start"]), int(p["sub"]), int(p["slot"])) for p in plan] == want
    rows = mutant_rows(ids, want, 1)
    assert ((rows != ids[None, :]).sum(1) == 1).all()            # every mutant differs from the read in exactly one base


def test_option_validation(built_lib):
    from chimeralm_amd import _native as N, explain as E

    ids = _read(10, 1)
    for kw in (dict(window=0), dict(stride=0), dict(window=2, stride=3), dict(substitute="X"), dict(substitute="all", window=2, stride=1),
               dict(substitute="all", window=2, stride=2), dict(score="logit"), dict(top_k=0), dict(top_k=33), dict(window=1.5),
               dict(stride=True)):
        with pytest.raises(ValueError):
            E.Options(**kw)
        with pytest.raises(ValueError):
            E.position_importance(None, ids, **kw)               # fails before anything touches a device
    with pytest.raises(ValueError):
        E.position_importance(None, ids, batch_size=0)
    E.Options(window=5, stride=5, substitute="N", score="gap", top_k=32)
    # the ABI refuses the same values with CLM_E_INVALID, and a read that is not bases + [SEP]
    lib = N.load()
    nm, nw = ctypes.c_int(), ctypes.c_int()

    def rc(arr, w, s, sub):
        return lib.clm_explain_plan(ctypes.c_void_p(arr.ctypes.data), arr.size, w, s, sub, None, 0, ctypes.byref(nm), ctypes.byref(nw))

    assert rc(ids, 1, 1, N.EXPLAIN_SUB_N) == 0 and (nm.value, nw.value) == (10, 10)
    for w, s, sub in ((0, 1, 0), (1, 0, 0), (2, 3, 0), (2, 1, N.EXPLAIN_SUB_ALL), (1, 1, 2)):
        assert rc(ids, w, s, sub) == N.E_INVALID
        assert lib.clm_explain_last_error(None)
    assert rc(ids[:-1].copy(), 1, 1, 0) == N.E_INVALID           # no [SEP]
    assert rc(np.array([1], np.uint8), 1, 1, 0) == N.E_INVALID   # no base
    padded = np.concatenate([np.array([4, 4], np.uint8), ids])
    assert rc(padded, 1, 1, 0) == N.E_INVALID                    # pads are stripped by the caller
    plan = np.zeros(4, dtype=E.PLAN_DTYPE)                       # a plan that does not fit its buffer
    assert lib.clm_explain_plan(ctypes.c_void_p(ids.ctypes.data), ids.size, 1, 1, 0, ctypes.c_void_p(plan.ctypes.data), 4,
                                ctypes.byref(nm), ctypes.byref(nw)) == N.E_INVALID and nm.value == 10
    with pytest.raises(ValueError):
        E.build_plan(padded)
    with pytest.raises(ValueError):
        E.tokenize(torch.zeros((2, 3), dtype=torch.int64))


def test_tokenize_as_predict_does():
    from chimeralm_amd import explain as E

    assert E.tokenize("ACGTN").tolist() == [7, 8, 9, 10, 11, 1]
    long = E.tokenize("A" * 40000)
    assert long.size == 32769 and long[-1] == 1 and (long[:-1] == 7).all()      # truncated to the tokenizer's maximum, [SEP] kept
    assert E.tokenize(torch.tensor([7, 8, 1])).dtype == np.uint8


def test_every_new_header_symbol_is_exported_and_bound(built_lib):
    from chimeralm_amd import _native as N

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    declared = set(re.findall(r"\b(clm_explain_[a-z_]+)\s*\(", header))
    assert declared == {"clm_explain_plan", "clm_explain_create", "clm_explain_rows", "clm_explain_scores", "clm_explain_reduce",
                        "clm_explain_last_error", "clm_explain_destroy"}
    lib = ctypes.CDLL(str(built_lib))
    for name in declared:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS
    from chimeralm_amd import build, explain as E

    assert "explain.hip" in build.SOURCES and E.PLAN_DTYPE.itemsize == ctypes.sizeof(N.ClmExplainMutant) == 16
    assert "#define CLM_ABI_VERSION 6" in header and N.ABI_VERSION == 6


def test_explain_kernels_have_no_scratch(built_lib):
    from chimeralm_amd import build

    text = build.RESOURCES.read_text()
    blocks = [b for b in text.split("Function Name: ")[1:] if "explain" in b.splitlines()[0]]
    names = [b.splitlines()[0] for b in blocks]
    assert sum("explain_reduce_kernel" in n for n in names) == 3 and any("explain_rows_kernel" in n for n in names) \
        and any("explain_scores_kernel" in n for n in names)
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1) == "0", b.splitlines()[0]


def test_cli_help_shows_the_options():
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "explain", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env={**os.environ, "PYTHONPATH": str(REPO), "COLUMNS": "200", "TERM": "dumb", "NO_COLOR": "1"},
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--output", "--max-reads", "--window", "--stride", "--substitute", "--score", "--top-k", "--values", "--weights", "--ckpt",
                "--precision"):
        assert opt in r.stdout, opt
    assert "fp16x3" in r.stdout and "noise floor" in " ".join(r.stdout.split())


def _fixed_importance():
    from chimeralm_amd.explain import Importance, Options

    logits = torch.tensor([[0.25, -0.5], [0.5, -0.25], [0.125, 0.0], [1.0, 2.0]], dtype=torch.float32)
    d = torch.tensor([[0.015625], [-0.25], [0.5]], dtype=torch.float32)
    return Importance(Options(window=2, stride=1, substitute="N", score="gap", top_k=4), 3, logits, d * 0.5, d,
                      torch.tensor([0.015625, 0.25, 0.5]), torch.tensor([2, 1, 0, -1], dtype=torch.int32),
                      torch.tensor([0.5, 0.25, 0.015625, 0.0]), torch.tensor([0], dtype=torch.int32))


def test_writer_bytes(tmp_path):
    from types import SimpleNamespace

    from chimeralm_amd.callbacks import ExplainWriter

    imp = _fixed_importance()
    w = ExplainWriter(tmp_path, values=True)
    tr = SimpleNamespace(global_rank=3)
    w.write_read(tr, "read/1", 0, imp)
    w.write_read(tr, "read/2", 1, imp)
    p1 = 1.0 / (1.0 + np.exp(0.75))
    line = f"\t0\t{p1:.6g}\t0.25\t-0.5\t3\t2\t1\tN\tgap\t2:0.5;1:0.25;0:0.015625\t0\n"
    assert (tmp_path / "3_explain.tsv").read_bytes() == ("read/1" + line + "read/2" + line).encode()
    raw = (tmp_path / "3_1.explain.npz").read_bytes()
    ExplainWriter(tmp_path / "again", values=True).write_read(tr, "read/2", 1, imp)
    assert (tmp_path / "again" / "3_1.explain.npz").read_bytes() == raw               # bytes depend on the arrays alone
    z = np.load(tmp_path / "3_1.explain.npz")
    assert z["name"].tolist() == ["read/2"] and sorted(z.files) == sorted(["name", "logits", "dp1", "dgap", "importance", "peak_pos",
                                                                     "peak_val", "n_nonfinite"])
    assert np.array_equal(z["importance"], imp.importance.numpy()) and z["peak_pos"].dtype == np.int32
    assert not list(tmp_path.glob("*.txt"))                                           # `filter` globs *.txt
    ExplainWriter(tmp_path).write_read(tr, "other", 0, imp)                           # a new writer starts the rank's file again
    assert (tmp_path / "3_explain.tsv").read_bytes() == ("other" + line).encode()
