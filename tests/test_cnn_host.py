"""DNAConvNet without a GPU: the fp64 helper against the reference module's golden outputs, the module's reference layout and
validation, the config route, the C ABI exports and the new kernels' compiler resources."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import cnn_reference as cr

REPO = Path(__file__).resolve().parent.parent
CFG = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
           hidden_dim=512, number_of_classes=2, dropout=0.1)
# reference cnn.py, production configuration: state_dict keys and shapes
REF_SHAPES = {"embedding.weight": (12, 256), "fc.0.weight": (512, 256), "fc.0.bias": (512,), "fc.4.weight": (2, 512),
              "fc.4.bias": (2,), "fc.1.num_batches_tracked": ()}
for _i in range(3):
    REF_SHAPES.update({f"conv_blocks.{_i}.0.weight": (256, 256, 7), f"conv_blocks.{_i}.0.bias": (256,),
                       f"conv_blocks.{_i}.1.num_batches_tracked": ()})
    REF_SHAPES.update({f"conv_blocks.{_i}.1.{s}": (256,) for s in ("weight", "bias", "running_mean", "running_var")})
REF_SHAPES.update({f"fc.1.{s}": (512,) for s in ("weight", "bias", "running_mean", "running_var")})


def test_fp64_helper_matches_the_reference_golden(golden_dir):
    g = np.load(golden_dir / "cnn_golden.npz")
    names = sorted({k.rsplit("_", 1)[0] for k in g.files})
    assert len(names) >= 5
    for name in names:
        seed, B, L, pads = (int(v) for v in g[f"{name}_meta"])
        tr = {}
        sd = cr.make_cnn_state_dict(seed)
        logits = cr.cnn_forward_fp64(sd, g[f"{name}_ids"], trace=tr).numpy()
        assert g[f"{name}_ids"].shape == (B, L)
        assert np.abs(logits - g[f"{name}_logits"]).max() < 1e-5, name
        assert np.abs(tr["pooled"].numpy() - g[f"{name}_pooled"]).max() < 1e-5, name
        assert 1.0 < np.abs(g[f"{name}_logits"]).max() < 10.0
    both = np.concatenate([g[f"{n}_logits"].argmax(1) for n in names])
    assert set(both.tolist()) == {0, 1}


def test_weights_exercise_the_traps():
    sd = cr.make_cnn_state_dict(0)
    for i in range(3):
        var, w = sd[f"conv_blocks.{i}.1.running_var"], sd[f"conv_blocks.{i}.1.weight"]
        assert 0.3 <= float(var.min()) and float(var.max()) <= 2.0 and (w < 0).any()
    assert float(sd["embedding.weight"][4].abs().max()) > 0.1          # the [PAD] row is not zero


def test_module_has_the_reference_state_dict_layout():
    from chimeralm_amd.cnn import DNAConvNet

    net = DNAConvNet(**CFG)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == REF_SHAPES
    assert net.number_of_classes == 2 and net.precision == "fp16x3"
    net.load_state_dict(cr.make_cnn_state_dict(1), strict=True)


def test_module_validation():
    from chimeralm_amd.cnn import DNAConvNet

    with pytest.raises(NotImplementedError):
        DNAConvNet(**{**CFG, "kernel_sizes": [5, 5, 5]})
    with pytest.raises(NotImplementedError):
        DNAConvNet(**{**CFG, "hidden_dim": 256})
    with pytest.raises(NotImplementedError):
        DNAConvNet(**{**CFG, "num_filters": [128, 256, 256]})
    for bad in ("fp16", "bf16", "fp16c", "f32"):
        with pytest.raises(ValueError):
            DNAConvNet(**CFG, precision=bad)
    assert DNAConvNet(**CFG, precision="fp32").precision == "fp32"
    with pytest.raises(RuntimeError, match="MI355X only"):
        DNAConvNet(**CFG)(torch.full((1, 100), 7, dtype=torch.int64))


def test_cnn_yaml_composes_and_instantiates(tmp_path):
    from chimeralm_amd.config import compose, instantiate

    bam = str(REPO / "tests/golden/test_chimric_reads.bam")
    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt", "model=cnn", f"+data.predict_data_path={bam}",
                                                    "model.net.precision=fp32"], output_dir=tmp_path)
    assert cfg.model.net._target_ == "chimeralm_amd.cnn.DNAConvNet"
    model = instantiate(cfg.model)
    assert type(model).__name__ == "ClassificationLit" and type(model.net).__name__ == "DNAConvNet"
    assert model.net.precision == "fp32" and model.net.number_of_classes == 2
    assert {k: tuple(v.shape) for k, v in model.net.state_dict().items()} == REF_SHAPES


def test_cnn_abi_is_exported(built_lib):
    from chimeralm_amd import _native

    lib = ctypes.CDLL(str(built_lib))
    for name in ("clm_cnn_create", "clm_cnn_load_weight", "clm_cnn_finalize", "clm_cnn_forward", "clm_cnn_debug_fetch",
                 "clm_cnn_last_error", "clm_cnn_destroy"):
        assert hasattr(lib, name) and name in _native.SYMBOLS
    assert lib.clm_abi_version() == _native.ABI_VERSION == 6
    hdr = (REPO / "include" / "chimeralm_hip.h").read_text()
    assert "#define CLM_ABI_VERSION 6" in hdr and "int clm_cnn_forward(" in hdr


def test_cnn_kernels_have_no_scratch(built_lib):
    from chimeralm_amd import build as B

    res, name = {}, None
    for ln in B.RESOURCES.read_text().splitlines():
        if ln.startswith("Function Name: "):
            name = ln.split(": ", 1)[1].strip()
            res[name] = {}
        elif name and ":" in ln:
            k, v = ln.strip().split(":", 1)
            res[name][k.strip()] = v.strip()
    hits = {n: r for n, r in res.items() if re.search(r"cnn_(gemm7|block0|head)_kernel", n)}
    assert len(hits) == 6, sorted(hits)                     # gemm7: {store, pooled sums} x {fp32, fp16x3}; block 0; head
    for n, r in hits.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, n
        if "gemm7" in n:
            assert int(r["Occupancy [waves/SIMD]"]) >= 2, n
