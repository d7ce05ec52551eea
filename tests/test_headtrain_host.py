"""Host side of the head fine-tune (no GPU): the pooling's backward formulas against fp64 autograd of the oracle's head, the C ABI's
three entry points, the backward kernel's registers, `fit_head`'s loop on a stub net with CPU tensors, and the errors the module and
the command line raise before anything touches a GPU."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import headtrain_reference as hr
from oracle import hyena_oracle as ho
from test_fit_host import PARQUET, _fit, _HostSums, _stub_model

REPO = Path(__file__).resolve().parent.parent
POOL_KEYS = ("attention.0.weight", "attention.0.bias", "attention.2.weight", "attention.2.bias")


# ------------------------------------------------------------------------------------------------ the formulas
def _autograd_case(B, L, w2_scale=1.0):
    """fp64 autograd of oracle.head_forward on seeded rows: (the formulas' gradients, autograd's) of the four pooling tensors."""
    c = hr.seeded_case(B, L, seed=3, w2_scale=w2_scale)
    sd = {k: v.double() for k, v in ho.make_state_dict(0).items()}
    for k, name in zip(POOL_KEYS, ("w1", "b1", "w2", "b2")):
        sd[ho.HD + k] = c[name].double().reshape(sd[ho.HD + k].shape).clone().requires_grad_(True)
    hidden = F.layer_norm(c["rows"].double(), (256,), c["lnf_g"].double(), c["lnf_b"].double(), ho.LN_EPS)
    trace = {}
    logits = ho.head_forward(hidden, sd, torch.float64, trace)
    trace["pooled"].retain_grad()
    F.cross_entropy(logits, torch.arange(B) % 2).backward()
    dpooled = trace["pooled"].grad
    fwd, grads = hr.pool_grads(c["rows"], c["lnf_g"], c["lnf_b"], c["w1"], c["b1"], c["w2"], c["b2"], dpooled, torch.float64)
    assert hr.rel_err(fwd["pooled"], trace["pooled"].detach()) <= 1e-12
    auto = [sd[ho.HD + k].grad for k in POOL_KEYS]
    return grads, auto


@pytest.mark.parametrize("B,L,w2_scale", [(2, 63, 1.0), (3, 65, 1.0), (2, 200, 1.0), (2, 200, 40.0)])
def test_formulas_match_fp64_autograd(B, L, w2_scale):
    grads, auto = _autograd_case(B, L, w2_scale)
    for name, got, want in zip(("dW1", "db1", "dw2"), grads, auto):
        err = hr.rel_err(got, want.reshape(got.shape))
        assert err <= 1e-12, f"{name} at ({B}, {L}) x{w2_scale}: {err:.3e}"
    # db2 is 0 in exact arithmetic; both sides return roundoff of the size of the other gradients' errors
    scale = float(auto[2].abs().max())
    assert abs(float(grads[3])) <= 1e-12 * scale and abs(float(auto[3])) <= 1e-12 * scale


def test_one_token_gives_exactly_zero():
    grads, auto = _autograd_case(1, 1)
    for got, want in zip(grads, auto):
        assert float(got.abs().max()) == 0.0 and float(want.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ ABI, registers
def test_abi_exports_the_entry_points(built_lib):
    from chimeralm_amd import _native as N

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    lib = N.load()
    for name in ("clm_rows", "clm_pool_forward", "clm_pool_backward"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in N.SYMBOLS
        assert hasattr(lib, name)
    assert lib.clm_abi_version() == N.ABI_VERSION == 6
    assert "#define CLM_ABI_VERSION 6" in header


def test_backward_kernel_registers(built_lib):
    from chimeralm_amd import build as B

    B.build()
    res, name = {}, None
    for ln in B.RESOURCES.read_text().splitlines():
        if ln.startswith("Function Name: "):
            name = ln.split(": ", 1)[1].strip()
            res[name] = {}
        elif name and ":" in ln:
            k, v = ln.strip().split(":", 1)
            res[name][k.strip()] = v.strip()
    hits = {n: r for n, r in res.items() if "pool_bwd_kernel" in n}
    assert len(hits) == 1, sorted(hits)
    for n, r in hits.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (n, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (n, r)


# ------------------------------------------------------------------------------------------------ fit_head on a stub net
def test_fit_head_on_a_stub_net(tmp_path):
    from chimeralm_amd import fit

    m2, h2 = _fit(tmp_path / "a", chunk_reads=2)
    m2b, h2b = _fit(tmp_path / "b", chunk_reads=2)
    m16, h16 = _fit(tmp_path / "c", chunk_reads=16)
    # micro-batches of two reads (18 = 8 + 8 + 2 reads per epoch -> 4 + 4 + 1 forwards) against the whole batch at once
    assert m2.net.seen[:9] == [2] * 9 and m16.net.seen[:3] == [8, 8, 2]
    strip = lambda h: [{k: v for k, v in r.items() if k != "seconds"} for r in h]   # noqa: E731
    assert strip(h2) == strip(h2b)                           # repeatable
    for a, b in zip(h2, h16):                                # the micro-batch shares add up to the batch's loss and gradient
        assert abs(a["train/loss"] - b["train/loss"]) <= 1e-12 and abs(a["val/loss"] - b["val/loss"]) <= 1e-12
    assert strip(_fit(tmp_path / "d", seed=7)[1]) != strip(h2)
    # metrics.tsv: the columns, one row per epoch
    lines = (tmp_path / "a" / "metrics.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(fit.METRIC_COLUMNS) == ["epoch", "train/loss", "train/f1", "val/loss", "val/f1", "lr", "seconds"]
    assert len(lines) == 3 and [ln.split("\t")[0] for ln in lines[1:]] == ["0", "1"]
    assert all(len(ln.split("\t")) == 7 for ln in lines[1:])
    assert h2[-1]["val/f1_best"] == max(r["val/f1"] for r in h2)


def test_unlabelled_reads_are_refused(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from chimeralm_amd import headtrain

    p = tmp_path / "plain.parquet"
    pq.write_table(pa.table({"id": ["r0|1", "r1"], "seq": ["ACGT", "GGCA"], "qual": ["IIII", "IIII"]}), str(p))
    with pytest.raises(ValueError, match="label"):
        headtrain.fit_head(_stub_model(), (str(p), 0, 2), (str(p), 0, 1), tmp_path / "o", epochs=1, device="cpu", metrics_factory=_HostSums)


# ------------------------------------------------------------------------------------------------ errors before any GPU work
def _hyena(**kw):
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    return HyenaDna(2, BinarySequenceClassifier(256), **kw)


def test_module_errors_without_a_gpu():
    from chimeralm_amd.basic_module import ClassificationLit

    ids = torch.full((2, 9), 7, dtype=torch.int64)
    net = _hyena(freeze_backbone=True, precision="fp16c").train()
    assert all(not p.requires_grad for p in net.backbone.parameters()) and all(p.requires_grad for p in net.head.parameters())
    with pytest.raises(ValueError, match=r"'fp32' or 'fp16x3'"):
        net(ids)
    # an unfrozen backbone does not train on this engine: the training step says so ...
    lit = ClassificationLit(net=_hyena(freeze_backbone=False, precision="fp32"))
    with pytest.raises(NotImplementedError, match=r"only the head trains on this engine: freeze_backbone=True"):
        lit.training_step({"input_ids": ids, "labels": torch.tensor([0, 1])})
    # ... and every call that was inference stays inference: eval() and no_grad of a frozen module take the old path (no CPU forward)
    with pytest.raises(RuntimeError, match="MI355X only"):
        _hyena(freeze_backbone=True, precision="fp32").eval()(ids)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X only"):
        _hyena(freeze_backbone=True, precision="fp32").train()(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):       # (the training path with CPU tensors: refused as well)
        _hyena(freeze_backbone=True, precision="fp32").train()(ids)


BAD_OPTIONS = [(["--precision", "fp16c"], "--precision must be fp16x3 or fp32"), (["--precision", "bf16"], "--precision must be fp16x3 or fp32"),
               (["--epochs", "0"], "--epochs must be"), (["-b", "0"], "--batch-size must be"), (["--lr", "0"], "--lr must be"),
               (["--val", "reads.bam"], "not in Parquet format"), (["--val", "nowhere.parquet"], "no such file"),
               (["--ckpt", "a.ckpt", "--weights", "dir"], "exclude each other"), (["--ckpt", "nowhere.ckpt"], "no such file")]


@pytest.mark.parametrize("args,said", BAD_OPTIONS)
def test_finetune_refuses_bad_options(args, said):
    """Refused by the command's own checks (their text), before a model is built or a GPU touched."""
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    res = CliRunner().invoke(app, ["finetune", str(PARQUET), *args], env={"COLUMNS": "250", "TERM": "dumb"})
    assert res.exit_code == 2, res.output
    assert said in " ".join(res.output.replace("│", " ").split()), res.output


def test_finetune_refuses_bad_files():
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    for path, said in (("reads.bam", "not in Parquet format"), ("missing.parquet", "no such file")):
        res = CliRunner().invoke(app, ["finetune", path], env={"COLUMNS": "250", "TERM": "dumb"})
        assert res.exit_code == 2 and said in " ".join(res.output.replace("│", " ").split()), res.output
