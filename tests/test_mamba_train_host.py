"""CPU tests of the Mamba training path (chimeralm_amd/mambatrain.py, csrc/mamba_train.hip): the hand formulas of the backward against
fp64 autograd, the ABI's new symbols, the module options, `fit_mamba` on a stub net and the `train --net` argument."""
from __future__ import annotations

import ctypes
import inspect
import re
from functools import partial
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import mamba_train_reference as R
from test_fit_host import PARQUET, _HostSums

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ("clm_mamba_train_create", "clm_mamba_train_workspace_bytes", "clm_mamba_train_forward", "clm_mamba_train_backward",
           "clm_mamba_train_last_error", "clm_mamba_train_destroy")
NAMES = ("out", "dzxbcdt") + R.CORE_PARAMS


def _worst(hand, auto):
    return {k: float((hand[k] - auto[k]).abs().max() / auto[k].abs().max().clamp_min(1e-300)) for k in NAMES if float(auto[k].abs().max()) > 0}


@pytest.mark.parametrize("L", [1, 63, 64, 65, 200])
def test_hand_formulas_against_autograd(L):
    """The chunked backward, gate + norm, softplus and conv + SiLU formulas in fp64 against torch autograd through the sequential
    scan: within 1e-10, the tolerance `scan_chunked` is held to (measured: <= 1e-14, dA_log included)."""
    zx, p, dout = R.random_core(L, 256, 1, 16, 2, L)
    hand = R.core_backward(zx, p, dout)
    auto = R.autograd_core(zx, p, dout, sequential=True)
    worst = _worst(hand, auto)
    print(worst)
    assert max(worst.values()) <= 1e-10, worst
    if L == 1:
        assert float(hand["A_log"].abs().max()) == 0.0 and float(auto["A_log"].abs().max()) == 0.0      # no decay acts on one token
    else:
        assert set(worst) == set(NAMES)
    # the sums of absolute terms bound what they stand for
    assert bool((hand["A_log_abs"] >= hand["A_log"].abs()).all()) and bool((hand["dt_bias_abs"] >= hand["dt_bias"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("shape", [(2, 64, 3, 65), (1, 128, 1, 130)])
def test_hand_formulas_on_other_shapes(shape):
    """More heads than one per state (expand 2) and the largest state, against autograd through the chunked scan."""
    expand, N, B, L = shape
    zx, p, dout = R.random_core(11, 256, expand, N, B, L)
    worst = _worst(R.core_backward(zx, p, dout), R.autograd_core(zx, p, dout))
    assert max(worst.values()) <= 1e-10, worst


def test_abi_exports_the_training_symbols(built_lib):
    from chimeralm_amd import _native

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    declared = {s for s in re.findall(r"\b(clm_[a-z_]+)\s*\(", header) if s.startswith("clm_mamba_train_")}
    assert declared == set(SYMBOLS)
    lib = ctypes.CDLL(str(built_lib))
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _native.SYMBOLS, name
    assert "#define CLM_ABI_VERSION 6" in header and _native.ABI_VERSION == 6
    from chimeralm_amd import build, mambatrain

    assert "mamba_train.hip" in build.SOURCES and mambatrain.N_PARAMS == 6 and "#define CLM_MAMBA_TRAIN_PARAMS 6" in header


def test_workspace_bytes_and_refusals_without_a_gpu(built_lib):
    """The size query needs no device: the formula of the header, CLM_E_INVALID for B < 1 or L < 1, CLM_E_UNSUPPORTED outside the
    supported shapes or beyond the index range."""
    from chimeralm_amd import _native as N
    from chimeralm_amd.mambatrain import workspace_bytes

    B, L, d, e, n = 8, 8193, 512, 3, 128
    di, H, cd, T = e * d, e * d // 64, e * d + 2 * n, (L + 63) // 64
    assert workspace_bytes(B, L, d, e, n) == 4 * (B * L * (2 * di + H + 2 * n * H) + B * T * (di + 5 * cd + H) + 2 * B * H)
    assert workspace_bytes(0, 5, 256, 1, 16) == N.E_INVALID and workspace_bytes(1, 0, 256, 1, 16) == N.E_INVALID
    for bad in ((1, 5, 384, 1, 16), (1, 5, 256, 1, 48), (1, 5, 256, 0, 16), (1 << 16, 1 << 15, 256, 1, 16)):
        assert workspace_bytes(*bad) == N.E_UNSUPPORTED, bad


def test_module_options():
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.mamba import MambaSequenceClassification, MambaSequenceClassificationSP

    sp = MambaSequenceClassificationSP(vocab_size=12, embedding_dim=256, number_of_layers=1, number_of_classes=2, dropout=0.1, d_state=16,
                                       expand=1, trainable=True)
    seq = MambaSequenceClassification(vocab_size=12, embedding_dim=256, number_of_layers=1, model_max_length=64, dropout=0.1,
                                      number_of_classes=2, d_state=16, expand=1)
    assert sp.trainable and not seq.trainable
    for cls in (MambaSequenceClassification, MambaSequenceClassificationSP):
        par = inspect.signature(cls.__init__).parameters["trainable"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    assert "trainable" not in "".join(sp.state_dict())                          # an option, not a tensor
    with pytest.raises(RuntimeError, match="MI355X only"):                      # no CPU path, training or not
        sp.train()(torch.zeros((1, 8), dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="only the head trains"):
        ClassificationLit(seq).train().training_step({"input_ids": torch.zeros((1, 8), dtype=torch.int64), "labels": torch.zeros(1)})


@pytest.mark.parametrize("name,opt,wd,patience", [("mamba", torch.optim.Adam, 0.0, 10), ("mambasp", torch.optim.AdamW, 0.01, 6)])
def test_yaml_has_the_reference_optimizer(name, opt, wd, patience, tmp_path):
    from chimeralm_amd.config import compose, instantiate

    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt", f"model={name}", "model.net.number_of_layers=1"], output_dir=tmp_path)
    model = instantiate(cfg.model)
    o = model.optimizer_factory(params=model.net.parameters())
    assert type(o) is opt and o.param_groups[0]["lr"] == 1e-4 and o.param_groups[0]["weight_decay"] == wd
    s = model.scheduler_factory(optimizer=o)
    assert type(s) is torch.optim.lr_scheduler.ReduceLROnPlateau and s.patience == patience and s.factor == 0.1
    assert not model.net.trainable
    assert instantiate(cfg.model.net, trainable=True).trainable


# ------------------------------------------------------------------------------------------------ the command's --net
def _invoke(args):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    res = CliRunner().invoke(app, ["train", str(PARQUET), *args], env={"COLUMNS": "250", "TERM": "dumb"})
    return res.exit_code, " ".join(res.output.replace("│", " ").split())


def test_train_net_argument():
    from chimeralm_amd.__main__ import TRAIN_NETS

    assert TRAIN_NETS == ("cnn", "mamba", "mambasp")
    code, out = _invoke(["--net", "hyena"])
    assert code == 2 and "--net must be one of cnn, mamba, mambasp" in out
    code, out = _invoke(["--net", "mambasp", "-b", "0"])
    assert code == 2 and "--batch-size must be 1 ... 65535" in out
    code, out = _invoke(["-b", "1"])                                            # the default net keeps BatchNorm's rule
    assert code == 2 and "BatchNorm needs two reads" in out
    code, out = _invoke(["--net", "mamba", "--epochs", "0"])
    assert code == 2 and "--epochs must be" in out
    code, out = _invoke(["--help"])
    assert code == 0 and "--net" in out and "mambasp" in out


# ------------------------------------------------------------------------------------------------ fit_mamba on a stub net
class _StubMamba(nn.Module):
    """Logits from the base composition of a read, on CPU tensors; every parameter trains."""

    def __init__(self):
        super().__init__()
        self.number_of_classes, self.trainable = 2, True
        self.fc = nn.Linear(16, 2)
        self.seen = []

    def forward(self, ids, quals=None):
        if self.training:
            self.seen.append(ids.shape[0])
        return self.fc(F.one_hot(ids, 16).double().mean(dim=1))


def _fit(tmp, batch_size, epochs=2, rows=17):
    from chimeralm_amd import mambatrain
    from chimeralm_amd.basic_module import ClassificationLit

    torch.manual_seed(0)
    model = ClassificationLit(net=_StubMamba().double(), optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                              scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=6))
    hist = mambatrain.fit_mamba(model, (str(PARQUET), 0, rows), (str(PARQUET), 18, 25), tmp, epochs=epochs, batch_size=batch_size, lr=1e-2,
                                device="cpu", metrics_factory=_HostSums)
    return model, hist


def test_fit_mamba_on_a_stub_net(tmp_path):
    from safetensors.torch import load_file

    from chimeralm_amd import fit, mambatrain

    m, h = _fit(tmp_path / "a", 8)
    assert m.net.seen == [8, 8, 1] * 2                                          # no two-read rule: the last read, alone, trains too
    m1, h1 = _fit(tmp_path / "b", 1, epochs=1, rows=5)
    assert m1.net.seen == [1] * 5 and len(h1) == 1
    mb, hb = _fit(tmp_path / "c", 8)
    strip = lambda hist: [{k: v for k, v in r.items() if k != "seconds"} for r in hist]   # noqa: E731
    assert strip(h) == strip(hb)
    lines = (tmp_path / "a" / "metrics.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(fit.METRIC_COLUMNS) and len(lines) == 3
    assert h[-1]["val/f1_best"] == max(r["val/f1"] for r in h)
    saved, own = load_file(str(tmp_path / "a" / "model.safetensors")), m.state_dict()
    assert sorted(saved) == sorted(own) and all(torch.equal(saved[k], own[k]) for k in own)
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        mambatrain.fit_mamba(m, (str(PARQUET), 0, 8), (str(PARQUET), 18, 25), tmp_path / "d", epochs=1, batch_size=0, device="cpu",
                             metrics_factory=_HostSums)
