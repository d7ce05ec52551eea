"""The Mamba nets without a GPU: the chunked fp64 scan against the recurrence, the fp64 helper against the reference modules'
golden outputs, the modules' reference layout and validation, the config routes, the C ABI exports and the new kernels' compiler
resources."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mamba_reference as mr

REPO = Path(__file__).resolve().parent.parent
CFG = {"mamba": dict(vocab_size=12, embedding_dim=256, number_of_layers=12, model_max_length=30000, dropout=0.1, d_state=16, d_conv=4,
                     expand=2, number_of_classes=2),
       "mambasp": dict(vocab_size=12, embedding_dim=512, number_of_layers=3, dropout=0.2, headdim=64, d_state=128, d_conv=4, expand=3,
                       number_of_classes=2)}
CLASSES = {"mamba": "MambaSequenceClassification", "mambasp": "MambaSequenceClassificationSP"}


def _net(variant, **kw):
    from chimeralm_amd import mamba

    return getattr(mamba, CLASSES[variant])(**{**CFG[variant], **kw})


def _ref_shapes(g, variant):
    return {str(k): tuple(int(s) for s in sh if s >= 0) for k, sh in zip(g[f"{variant}_keys"], g[f"{variant}_shapes"])}


@pytest.mark.parametrize("L", [1, 63, 64, 65, 300])
def test_chunked_scan_equals_the_recurrence(L):
    g = torch.Generator().manual_seed(L)
    B, H, P, N = 2, 3, 16, 8
    x = torch.randn(B, L, H, P, generator=g, dtype=torch.float64)
    dt = torch.nn.functional.softplus(torch.randn(B, L, H, generator=g, dtype=torch.float64) - 2.0) * 3.0   # up to ~10: dt A to -160
    A = -torch.rand(H, generator=g, dtype=torch.float64) * 15.0 - 1.0
    Bm, Cm = torch.randn(B, L, N, generator=g, dtype=torch.float64), torch.randn(B, L, N, generator=g, dtype=torch.float64)
    Dv = torch.rand(H, generator=g, dtype=torch.float64)
    seq = mr.scan_sequential(x, dt, A, Bm, Cm, Dv)
    for Q in (64, 16):
        ch = mr.scan_chunked(x, dt, A, Bm, Cm, Dv, Q=Q)
        assert torch.isfinite(ch).all()
        assert float((ch - seq).abs().max()) <= 1e-10 * max(1.0, float(seq.abs().max())), (L, Q)


def test_fp64_helper_matches_the_reference_golden(golden_dir):
    g = np.load(golden_dir / "mamba_golden.npz")
    names = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_meta")})
    assert len(names) == 16
    for name in names:
        var, seed, B, L, pads, d_state, masked = (int(v) for v in g[f"{name}_meta"])
        variant = ("mamba", "mambasp")[var]
        sd = mr.make_mamba_state_dict(variant, seed, d_state=d_state)
        tr = {}
        mask = g[f"{name}_mask"] if masked else None
        logits = mr.mamba_forward_fp64(variant, sd, g[f"{name}_ids"], mask=mask, trace=tr).numpy()
        assert g[f"{name}_ids"].shape == (B, L)
        assert np.abs(logits - g[f"{name}_logits"]).max() < 1e-6, name
        assert np.abs(tr["pooled"].numpy() - g[f"{name}_pooled"]).max() < 1e-6, name
        assert np.abs(g[f"{name}_logits"]).max() < 25.0, name
    assert np.median([np.abs(g[f"{n}_logits"]).max() for n in names]) > 1.0        # O(1) logits, not vacuous ones
    both = np.concatenate([g[f"{n}_logits"].argmax(1) for n in names])
    assert set(both.tolist()) == {0, 1}


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_modules_have_the_reference_state_dict_layout(golden_dir, variant):
    g = np.load(golden_dir / "mamba_golden.npz")
    net = _net(variant)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == _ref_shapes(g, variant)
    assert net.number_of_classes == 2 and net.precision == "fp16x3"
    assert not hasattr(net, "_engine")
    net.load_state_dict(mr.make_mamba_state_dict(variant, 1), strict=True)
    lay = net.mamba_layers[0]["mamba"] if variant == "mamba" else net.mamba_layers[0]
    A = torch.exp(lay.A_log.detach())
    assert float(A.min()) >= 1.0 and float(A.max()) <= 16.0


def test_mamba2_container_initialisation():
    from chimeralm_amd.mamba import Mamba2

    torch.manual_seed(0)
    m = Mamba2(512, d_state=128, expand=3)
    A = torch.exp(m.A_log.detach())
    dt = torch.nn.functional.softplus(m.dt_bias.detach())
    assert m.nheads == 24 and 1.0 <= float(A.min()) and float(A.max()) <= 16.0
    assert 1e-4 <= float(dt.min()) and float(dt.max()) <= 0.1 + 1e-6
    assert torch.equal(m.D.detach(), torch.ones(24)) and torch.equal(m.norm.weight.detach(), torch.ones(1536))
    assert tuple(m.in_proj.weight.shape) == (3352, 512) and m.in_proj.bias is None and m.out_proj.bias is None


def test_module_validation():
    for variant in ("mamba", "mambasp"):
        for bad in (dict(headdim=32), dict(d_state=8), dict(embedding_dim=384), dict(d_conv=3), dict(number_of_classes=3),
                    dict(vocab_size=16)):
            with pytest.raises(NotImplementedError):
                _net(variant, **bad)
        for bad in ("fp16", "bf16", "fp16c", "f32"):
            with pytest.raises(ValueError):
                _net(variant, precision=bad)
        assert _net(variant, precision="fp32", number_of_layers=1).precision == "fp32"
        with pytest.raises(RuntimeError, match="MI355X only"):
            _net(variant, number_of_layers=1)(torch.full((1, 100), 7, dtype=torch.int64))


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_yaml_composes_and_instantiates(tmp_path, golden_dir, variant):
    from chimeralm_amd.config import compose, instantiate

    bam = str(REPO / "tests/golden/test_chimric_reads.bam")
    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt", f"model={variant}", f"+data.predict_data_path={bam}",
                                                    "model.net.precision=fp32"], output_dir=tmp_path)
    assert cfg.model.net._target_ == f"chimeralm_amd.mamba.{CLASSES[variant]}"
    model = instantiate(cfg.model)
    assert type(model).__name__ == "ClassificationLit" and type(model.net).__name__ == CLASSES[variant]
    assert model.net.precision == "fp32" and model.net.number_of_classes == 2
    g = np.load(golden_dir / "mamba_golden.npz")
    assert {k: tuple(v.shape) for k, v in model.net.state_dict().items()} == _ref_shapes(g, variant)


def test_mamba_abi_is_exported(built_lib):
    from chimeralm_amd import _native

    lib = ctypes.CDLL(str(built_lib))
    hdr = (REPO / "include" / "chimeralm_hip.h").read_text()
    for name in ("clm_mamba_create", "clm_mamba_load_weight", "clm_mamba_finalize", "clm_mamba_forward", "clm_mamba_debug_fetch",
                 "clm_mamba_last_error", "clm_mamba_destroy"):
        assert hasattr(lib, name) and name in _native.SYMBOLS and f"{name}(" in hdr
    assert lib.clm_abi_version() == _native.ABI_VERSION == 6
    assert "#define CLM_MAMBA_SEQ 0" in hdr and "#define CLM_MAMBA_SP 1" in hdr


def test_mamba_create_rejects_unsupported_shapes(built_lib):
    """Shape checks run before any device is touched, so they answer without a GPU."""
    from chimeralm_amd import _native as N

    lib = N.load()
    h = ctypes.c_void_p()
    for args in [(N.MAMBA_SP, N.PREC_F32, 384, 3, 128, 3, 64, 0), (N.MAMBA_SP, N.PREC_F32, 512, 3, 48, 3, 64, 0),
                 (N.MAMBA_SP, N.PREC_F32, 512, 3, 128, 3, 32, 0), (N.MAMBA_SEQ, N.PREC_F32, 256, 12, 16, 2, 64, 0),
                 (N.MAMBA_SP, N.PREC_F16C, 512, 3, 128, 3, 64, 0), (7, N.PREC_F32, 512, 3, 128, 3, 64, 0)]:
        assert lib.clm_mamba_create(0, *args, ctypes.byref(h)) == -1, args
        assert lib.clm_mamba_last_error(None).decode().startswith("clm_mamba_create")


def test_mamba_kernels_have_no_scratch(built_lib):
    from chimeralm_amd import build as B

    res, name = {}, None
    for ln in B.RESOURCES.read_text().splitlines():
        if ln.startswith("Function Name: "):
            name = ln.split(": ", 1)[1].strip()
            res[name] = {}
        elif name and ":" in ln:
            k, v = ln.strip().split(":", 1)
            res[name][k.strip()] = v.strip()
    hits = {n: r for n, r in res.items() if re.search(r"mamba_[a-z_]+_kernel", n)}
    # proj: {front, in_proj, out_proj, out_proj + pooling} x {fp32, fp16x3}; scan: d_state 16 / 32 / 64 / 128; conv; front LN x 2;
    # embed; head x 2 (d_model 256 and 512)
    assert len(hits) == 18, sorted(hits)
    for n, r in hits.items():
        # the d_state-128 scan keeps about 44 loop-invariant addresses in scratch at two waves per SIMD (stored once in the
        # prologue, each reloaded once per 64-token chunk, against ~350 MFMAs per wave and chunk); every other kernel has none
        allowed = 192 if "mamba_scan_kernelILi128E" in n else 0
        assert int(r["ScratchSize [bytes/lane]"]) <= allowed, n
        if "mamba_proj_kernel" in n or "mamba_scan_kernel" in n:
            assert int(r["Occupancy [waves/SIMD]"]) >= 2, n
    # the existing kernels' name patterns do not catch the new ones
    for pat in (r"cnn_(gemm7|block0|head)_kernel", r"conv32_kernel", r"(tail|enc)32_kernel", r"hyena_conv_pers_kernel", r"attention_x3_kernel"):
        assert not any(re.search(pat, n) for n in hits), pat
