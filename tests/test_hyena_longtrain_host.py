"""The segmented Hyena training core on the CPU (tests/hyena_longtrain_reference.py, chimeralm_amd/hyenatrain.py): the segment
formulas against the dense fp64 sums, the ABI's three new symbols, the workspace formula and the refusals, the module's and the
command's new option, and which core a batch takes."""
from __future__ import annotations

import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import hyena_longtrain_reference as LR
import hyena_train_reference as R

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ("clm_hyena_longtrain_workspace_bytes", "clm_hyena_longtrain_forward", "clm_hyena_longtrain_backward")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("PL", [(8, 1), (8, 5), (8, 8), (8, 9), (8, 16), (8, 17), (8, 29), (8, 33), (64, 129), (64, 200)])
def test_segment_formulas_match_the_dense_sums(PL):
    """One segment, a full one, a lone token after one and after two, ragged ends, up to five segments; 2 reads."""
    P, L = PL
    args = R.random_core(20 + L, 2, L, torch.float64, channels=4)
    want, got = R.hand_core(*args), LR.segmented_core(*args, P=P)
    assert set(got) == set(R.fft_core(*args)) and set(got["den"]) == set(want["den"])
    for k in ("c", "y", "dg") + R.CORE_GRADS:
        assert _rel(got[k], want[k]) <= 1e-12, (k, _rel(got[k], want[k]))
    for k, den in want["den"].items():
        assert _rel(got["den"][k], den) <= 1e-12, k


def test_abi_carries_the_three_symbols_at_version_6(built_lib):
    from chimeralm_amd import _native as N

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    assert re.search(r"#define CLM_ABI_VERSION 6\b", header) and N.ABI_VERSION == 6
    lib = N.load()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\(", header), sym
        assert sym in N.SYMBOLS and hasattr(lib, sym)
    assert N.SYMBOLS["clm_hyena_longtrain_forward"] == N.SYMBOLS["clm_hyena_train_forward"]
    assert N.SYMBOLS["clm_hyena_longtrain_backward"] == N.SYMBOLS["clm_hyena_train_backward"]


def test_workspace_formula_and_refusals(built_lib):
    from chimeralm_amd import _native as N
    from chimeralm_amd import hyenatrain as ht

    lib = N.load()
    f = lib.clm_hyena_longtrain_workspace_bytes
    for B, L in [(1, 1), (1, 8192), (1, 8193), (1, 8194), (2, 16384), (1, 16385), (2, 32769)]:
        assert f(B, L) == LR.workspace_bytes(B, L) == ht.long_workspace_bytes(B, L), (B, L)
    assert f(1, 8194) == (4 * (16384 + 512 * 2 * 8193 + 1024 * 2 * 8193 + 256 * 8194 + 256 * 16) + 15) // 16 * 16
    assert [LR.segments(L) for L in (1, 8192, 8193, 16384, 16385, 32768, 32769)] == [1, 1, 2, 2, 3, 4, 5]
    assert f(0, 5) == N.E_INVALID and f(1, 0) == N.E_INVALID and f(-1, -1) == N.E_INVALID and f(65536, 5) == N.E_INVALID
    assert f(65535, 1) > 0
    assert f(1, 32770) == N.E_UNSUPPORTED and f(2, 40000) == N.E_UNSUPPORTED
    assert ht.MAX_LONG_TOKENS == LR.MAX_TOKENS == 32769
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED"):
        ht.long_workspace_bytes(1, 32770)
    # the old op still refuses what it refused
    assert lib.clm_hyena_train_workspace_bytes(1, 8194) == N.E_UNSUPPORTED
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED"):
        ht.workspace_bytes(1, 8194)


def test_refused_calls_launch_nothing(built_lib):
    """Every refusal comes back before the first HIP call: these run without a GPU, on pointers that are never followed."""
    from chimeralm_amd import _native as N

    lib = N.load()
    ok = 4096                                                            # non-NULL, on 4 bytes
    fwd, bwd = lib.clm_hyena_longtrain_forward, lib.clm_hyena_longtrain_backward
    fa = lambda ptrs, B=1, L=9: fwd(*ptrs[:5], B, L, *ptrs[5:8], None)    # noqa: E731
    ba = lambda ptrs, B=1, L=9: bwd(*ptrs[:7], B, L, *ptrs[7:13], None)   # noqa: E731
    for call, n in ((fa, 8), (ba, 13)):
        assert call([ok] * n, L=32770) == N.E_UNSUPPORTED
        assert call([ok] * n, B=0) == N.E_INVALID and call([ok] * n, L=0) == N.E_INVALID and call([ok] * n, B=65536) == N.E_INVALID
        for i in range(n):
            for bad in (None, ok + 2):
                ptrs = [ok] * n
                ptrs[i] = bad
                assert call(ptrs) == N.E_INVALID, (n, i, bad)


def test_module_option():
    from chimeralm_amd import lm
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    p = inspect.signature(HyenaDna.__init__).parameters["hyena_long_core"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "torch"
    for fn in (lm.ChimeraLM.new, lm.ChimeraLM.from_pretrained):
        q = inspect.signature(fn).parameters["hyena_long_core"]
        assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default == "torch"
    plain = HyenaDna(2, BinarySequenceClassifier(256))
    net = HyenaDna(2, BinarySequenceClassifier(256), trainable=True, hyena_long_core="engine")
    assert (plain.hyena_long_core, net.hyena_long_core, net.hyena_core) == ("torch", "engine", "engine")
    assert list(net.state_dict()) == list(plain.state_dict()) and not any("long_core" in k for k in net.state_dict())
    with pytest.raises(ValueError, match="hyena_long_core"):
        HyenaDna(2, BinarySequenceClassifier(256), hyena_long_core="fft")
    lit = lm.ChimeraLM.new(trainable=True, hyena_long_core="engine")
    assert lit.net.hyena_long_core == "engine" and lit.net.hyena_core == "engine"


def test_finetune_refuses_a_bad_long_core(golden_dir, tmp_path):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    r = CliRunner().invoke(app, ["finetune", str(golden_dir / "tests.parquet"), "-o", str(tmp_path / "o"), "--train-backbone",
                                 "--hyena-long-core", "fft"])
    assert r.exit_code == 2 and "--hyena-long-core must be torch or engine" in r.output
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("core", ["engine", "torch"])
@pytest.mark.parametrize("long_core", ["torch", "engine"])
@pytest.mark.parametrize("L", [8193, 8194, 32769, 32770])
def test_which_core_a_batch_takes(core, long_core, L):
    from chimeralm_amd import hyenatrain as ht

    net = SimpleNamespace(hyena_core=core, hyena_long_core=long_core)
    if core == "torch" or L > 32769:
        want = "torch"
    elif L <= 8193:
        want = "engine"
    else:
        want = "engine-long" if long_core == "engine" else "torch"
    assert ht._core_for(net, L, SimpleNamespace(type="cuda")) == want
    if want == "torch":
        assert ht._core_for(net, L, torch.device("cpu")) == "torch"
    else:
        with pytest.raises(RuntimeError, match="hyena_core"):
            ht._core_for(net, L, torch.device("cpu"))
