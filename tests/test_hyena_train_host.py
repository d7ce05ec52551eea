"""The Hyena training core on the CPU (tests/hyena_train_reference.py, chimeralm_amd/hyenatrain.py): the written formulas and both
circular forms against fp64 autograd, one training step of the whole net on the torch core against fp64 autograd through the oracle,
the ABI's three symbols and the workspace formula, the module's two options and the command's option check."""
from __future__ import annotations

import inspect
import re
from pathlib import Path

import pytest
import torch

import hyena_train_reference as R
from oracle import hyena_oracle as ho

REPO = Path(__file__).resolve().parent.parent
FLOOR = 32 * 2.0 ** -24


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("BL", [(2, 1), (2, 2), (3, 3), (3, 129), (2, 130)])
def test_hand_formulas_match_fp64_autograd(BL):
    B, L = BL
    args = R.random_core(L, B, L, torch.float64, channels=4)
    auto = R.autograd_core(*args)
    for name, fn in (("dense", R.hand_core), ("fft", R.fft_core)):
        hand = fn(*args)
        for k in ("y",) + R.CORE_GRADS:
            assert _rel(hand[k], auto[k]) <= 1e-12, (name, k, _rel(hand[k], auto[k]))
        for k, den in hand["den"].items():                           # the sums of absolute terms bound the sums
            assert bool((den >= hand[k].abs() * (1 - 1e-9)).all()), (name, k)


@pytest.mark.parametrize("BL", [(2, 2), (3, 3), (3, 129), (2, 130), (1, 200)])
def test_circular_forms_match_the_formulas(BL):
    """N = 2 L - 2 (one wrapped product in c, dg and dk, subtracted) and a roomier N: reads packed in pairs with the Re identity for
    dk, odd and even B; and the kernels' form, two sequences of one read separated through the mirrored bin."""
    B, L = BL
    args = R.random_core(10 + L, B, L, torch.float64, channels=4)
    want = R.hand_core(*args)
    for n in (None, 256 if L <= 129 else 512):
        for name, fn in (("pairs", R.circular_pairs), ("mirror", R.circular_mirror)):
            got = fn(*args, n=n)
            for k in ("c", "dg", "dk"):
                assert _rel(got[k], want[k]) <= 1e-12, (name, n, k, _rel(got[k], want[k]))


def test_alias_corrections_are_needed():
    args = R.random_core(3, 2, 129, torch.float64, channels=4)
    want, got = R.hand_core(*args), R.circular_mirror(*args, n=256)
    zc, sw, sb, k, D, dy = args
    u, _ = R._short(zc, sw, sb)
    g = u[:, 8:] * u[:, 4:8]
    assert _rel(got["c"], want["c"]) <= 1e-12
    wrapped = got["c"].clone()
    wrapped[..., 0] += g[..., 128] * k[..., 128]                     # what the transform alone gives
    assert _rel(wrapped, want["c"]) > 1e-3


# ------------------------------------------------------------------------------------------------------------- the net on the CPU
def _module(sd, dropout=0.0, **kw):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    net = HyenaDna(2, BinarySequenceClassifier(256, dropout=dropout), precision="fp32", selfcheck=False, **kw)
    net.embed_dropout = dropout
    lit = ClassificationLit(net=net)
    lit.load_state_dict(sd, strict=True)
    return lit


def test_training_step_on_the_cpu():
    """One training_step at 3 x 203 (17 left pads on read 0, dropout 0), torch core, float32 on CPU tensors, against fp64 autograd
    through the oracle on the same weights: loss, logits and p.grad of every parameter within max(8 x the oracle's own float32 error,
    32 x 2^-24) of each tensor's maximum."""
    sd = ho.make_state_dict(0)
    ids, labels = R.step_batch()
    r64, r32 = R.net_step(sd, ids, labels, torch.float64), R.net_step(sd, ids, labels, torch.float32)
    lit = _module(sd, trainable=True, hyena_core="torch").train()
    seen = {}
    hook = lit.net.head.output_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach()))
    loss = lit.training_step({"input_ids": ids, "labels": labels})
    loss.backward()
    hook.remove()
    assert lit.net.last_train_core == "torch"
    grads = {k: p.grad for k, p in lit.net.named_parameters()}
    assert set(grads) == set(r64["grads"])                           # (named_parameters lists the shared freq once)
    assert all(g is not None for g in grads.values())
    items = [("loss", loss.detach(), r64["loss"], r32["loss"]), ("logits", seen["logits"], r64["logits"], r32["logits"])]
    items += [(k, grads[k], r64["grads"][k], r32["grads"][k]) for k in sorted(grads)]
    bad = []
    for name, got, w64, w32 in items:
        den = float(r64["den"].get(name, w64).abs().max().clamp_min(1e-300))     # (the score bias: a sum that cancels to 0)
        err, err32 = float((got.double() - w64).abs().max()) / den, float((w32.double() - w64).abs().max()) / den
        line = f"{name:70s} cpu-fp32 module {err:.3e}  oracle fp32 {err32:.3e}  bound {max(8 * err32, FLOOR):.3e}"
        print(line)
        if not err <= max(8 * err32, FLOOR):
            bad.append(line)
    assert not bad, "\n".join(bad)
    z = grads["backbone.backbone.layers.0.mixer.filter_fn.pos_emb.z"]
    assert float(z[:, :203].abs().max()) > 0 and float(z[:, 203:].abs().max()) == 0.0
    f = lit.net.backbone.backbone.layers[0].mixer.filter_fn.implicit_filter
    assert f[1].freq is f[3].freq and f[3].freq is f[5].freq


def test_engine_core_refuses_cpu_tensors():
    sd = ho.make_state_dict(0)
    ids, labels = R.step_batch(B=1, L=9, pads=0)
    lit = _module(sd, trainable=True).train()
    with pytest.raises(RuntimeError, match="hyena_core"):
        lit.training_step({"input_ids": ids, "labels": labels})


# ------------------------------------------------------------------------------------------------------------- ABI and options
def test_abi_carries_the_three_symbols_at_version_6(built_lib):
    from chimeralm_amd import _native as N

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    assert re.search(r"#define CLM_ABI_VERSION 6\b", header) and N.ABI_VERSION == 6
    for sym in ("clm_hyena_train_workspace_bytes", "clm_hyena_train_forward", "clm_hyena_train_backward"):
        assert re.search(rf"\b{sym}\(", header), sym
        assert sym in N.SYMBOLS
    lib = N.load()
    f = lib.clm_hyena_train_workspace_bytes
    assert f(0, 5) == N.E_INVALID and f(1, 0) == N.E_INVALID and f(-1, -1) == N.E_INVALID
    assert f(1, 8194) == N.E_UNSUPPORTED and f(2, 40000) == N.E_UNSUPPORTED
    for B, L in [(1, 1), (2, 2), (3, 129), (2, 130), (2, 513), (2, 700), (2, 1031), (1, 4097), (2, 8000), (8, 8193)]:
        assert f(B, L) == R.workspace_bytes(B, L), (B, L)
    assert f(3, 129) == (4 * (256 + 512 * 129 + 3 * 256 * 129 + 3 * 256 * 16) + 15) // 16 * 16
    assert [R.logn_for(L) for L in (1, 129, 130, 513, 700, 1031, 4097, 8000, 8193, 8194)] == [8, 8, 9, 10, 11, 12, 13, 14, 14, -1]


def test_module_options():
    from chimeralm_amd import lm
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    sig = inspect.signature(HyenaDna.__init__).parameters
    for name, default in (("trainable", False), ("hyena_core", "engine")):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
        for fn in (lm.ChimeraLM.new, lm.ChimeraLM.from_pretrained):
            p = inspect.signature(fn).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
    plain = HyenaDna(2, BinarySequenceClassifier(256))
    net = HyenaDna(2, BinarySequenceClassifier(256), trainable=True, hyena_core="torch")
    assert (net.trainable, net.hyena_core, plain.trainable, plain.hyena_core) == (True, "torch", False, "engine")
    assert list(net.state_dict()) == list(plain.state_dict())
    assert not any("trainable" in k or "hyena_core" in k or "dropout" in k for k in net.state_dict())
    with pytest.raises(ValueError, match="hyena_core"):
        HyenaDna(2, BinarySequenceClassifier(256), hyena_core="fft")
    lit = lm.ChimeraLM.new(trainable=True, hyena_core="torch")
    assert lit.net.trainable and lit.net.hyena_core == "torch" and not lit.net.freeze_backbone


def test_finetune_refuses_a_bad_core(golden_dir, tmp_path):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    r = CliRunner().invoke(app, ["finetune", str(golden_dir / "tests.parquet"), "-o", str(tmp_path / "o"), "--train-backbone",
                                 "--hyena-core", "fft"])
    assert r.exit_code == 2 and "--hyena-core must be engine or torch" in r.output
    assert not (tmp_path / "o").exists()
