"""Host side of DNAConvNet training (no GPU): the restated formulas (tests/cnn_train_reference.py) against the reference class's own
training step (tests/golden/cnn_train_golden.npz), the ABI, `training_step`'s outcomes, the `train` command's option checks and
`fit_cnn` on a stub net with CPU tensors.
"""
from __future__ import annotations

import ctypes
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import cnn_reference as cr
import cnn_train_reference as ctr
from test_fit_host import PARQUET, _HostSums

REPO = Path(__file__).resolve().parent.parent
CFG = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4], hidden_dim=512,
           number_of_classes=2, padding_idx=4)
# the worst relative difference (max |restated fp64 - reference class fp32| / max |reference class|) over a case's tensors, measured
# when the golden was made, x 4 for another BLAS
TOLERANCE = {"l64": 4 * 4.0e-4, "l67": 4 * 2.3e-5, "l203pad": 4 * 7.9e-6, "l1031pad": 4 * 9.3e-6}
SYMBOLS = ("clm_cnn_train_create", "clm_cnn_train_workspace_bytes", "clm_cnn_train_forward", "clm_cnn_train_generation",
           "clm_cnn_train_backward", "clm_cnn_train_debug_fetch", "clm_cnn_train_last_error", "clm_cnn_train_destroy")


def _rel(a, b) -> float:
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", sorted(TOLERANCE))
def test_restated_formulas_against_the_reference_class(name, golden_dir):
    """One training step of the reference's own DNAConvNet (train(), dropout 0, fp32) against the same step restated in fp64.
    Measured worst per case: l64 4.0e-4 (a batch of 2 makes fc's BatchNorm ill-conditioned), l67 2.3e-5, l203pad 7.9e-6, l1031pad
    9.3e-6.  Biases in front of a BatchNorm have gradient 0 in exact arithmetic: the class's fp32 leaves up to 8.1e-5 there, the
    restatement 4e-15, and both are held below 1e-3 of the largest gradient of the BatchNorm's own bias."""
    g = np.load(golden_dir / "cnn_train_golden.npz")
    seed, B, L, pads = g[f"{name}_meta"].tolist()
    r = ctr.cnn_train_reference(cr.make_cnn_state_dict(seed), cr.synthetic_ids(seed, B, L, pads), ctr.synthetic_labels(seed, B), torch.float64)
    tol, seen = TOLERANCE[name], 0
    for k in g.files:
        if not k.startswith(name + "_") or k.endswith("_meta"):
            continue
        kind, _, key = k[len(name) + 1:].partition(":")
        if kind in ("loss", "logits"):
            err = _rel(r[kind], g[k])
        elif kind == "g" and key.endswith(".0.bias"):
            after = key.replace(".0.bias", ".1.bias")
            limit = 1e-3 * float(np.abs(g[f"{name}_g:{after}"]).max())
            assert float(np.abs(g[k]).max()) <= limit and float(r["grads"][key].abs().max()) <= limit, k
            continue
        elif kind == "g":
            err = _rel(r["grads"][key], g[k])
        elif kind == "gs":
            got = r["grads"][key][:8][:, :, [0, 3, 6]]
            err = float((got - torch.from_numpy(g[k]).double()).abs().max() / float(g[f"{name}_gmax:{key}"]))
        elif kind == "gmax":
            err = abs(float(r["grads"][key].abs().max()) - float(g[k])) / float(g[k])
        elif key.endswith("num_batches_tracked"):
            assert int(r["running"][key]) == int(g[k]) == 1001
            continue
        else:
            err = _rel(r["running"][key], g[k])
        seen += 1
        assert err <= tol, (k, err, tol)
    assert seen == 2 + 10 + 3 + 3 + 8                       # loss, logits | full gradients | conv slices | their max-abs | running
    assert bool((r["grads"]["embedding.weight"][4] == 0).all()) and not np.abs(g[f"{name}_g:embedding.weight"][4]).any()
    # the running variance follows the unbiased rule, n / (n - 1) of the biased batch variance: plain to see at fc.1, where n = B
    old = cr.make_cnn_state_dict(seed)["fc.1.running_var"].double()
    assert _rel(0.9 * old + 0.1 * r["fc_var"] * B / (B - 1), g[f"{name}_r:fc.1.running_var"]) <= tol
    assert _rel(0.9 * old + 0.1 * r["fc_var"], g[f"{name}_r:fc.1.running_var"]) > 10 * tol


def test_choice_routes_the_pool():
    """A given choice replaces torch's own: the lowest index on ties by default, and the gradient follows whatever is handed in."""
    sd, ids, labels = cr.make_cnn_state_dict(2), cr.synthetic_ids(2, 3, 203, 17), ctr.synthetic_labels(2, 3)
    free = ctr.cnn_train_reference(sd, ids, labels, torch.float64)
    assert int(free["choice"][0][:, 1:3].max()) == 0          # positions 4 .. 11 see nothing but the 17 pads: four equal values, index 0
    same = ctr.cnn_train_reference(sd, ids, labels, torch.float64, choice=[c.numpy() for c in free["choice"]])
    assert torch.equal(same["loss"], free["loss"]) and all(torch.equal(same["grads"][k], free["grads"][k]) for k in ctr.PARAM_KEYS)
    moved = [c.numpy().copy() for c in free["choice"]]
    moved[0][:, 1:3] = 3                                     # another of the equal values: the same loss, the gradient elsewhere
    other = ctr.cnn_train_reference(sd, ids, labels, torch.float64, choice=moved)
    assert torch.equal(other["loss"], free["loss"]) and not torch.equal(other["dz"][0], free["dz"][0])


def test_abi_is_exported_and_bound(built_lib):
    from chimeralm_amd import _native, build

    lib = ctypes.CDLL(str(built_lib))
    hdr = (REPO / "include" / "chimeralm_hip.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _native.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert lib.clm_abi_version() == _native.ABI_VERSION == 6 and "#define CLM_ABI_VERSION 6" in hdr
    assert "#define CLM_CNN_TRAIN_PARAMS 13" in hdr and "choice[b, j, c] = the LOWEST r" in hdr
    assert "cnn_train.hip" in build.SOURCES
    lib.clm_cnn_train_workspace_bytes.restype = ctypes.c_int64
    assert lib.clm_cnn_train_workspace_bytes(8, 8193) > 8 * 8193 * 256 * 4 * 2 and lib.clm_cnn_train_workspace_bytes(8, 63) < 0
    # the new kernels keep their names out of the patterns of tests/test_kernel_resources.py, and none of them spills
    names = [ln.split("Function Name: ", 1)[1] for ln in build.RESOURCES.read_text().splitlines() if "Function Name:" in ln and "cnn_train_" in ln]
    assert len(names) >= 15
    res, cur = {}, None
    for ln in build.RESOURCES.read_text().splitlines():
        if "Function Name:" in ln:
            cur = ln.split("Function Name: ", 1)[1]
        elif "ScratchSize" in ln and cur in names:
            res[cur] = int(ln.split(":")[1].strip())
    assert res and not any(res.values()), res


def test_training_step_outcomes():
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.cnn import DNAConvNet
    from test_headtrain_host import _hyena

    batch = {"input_ids": torch.full((2, 100), 7, dtype=torch.int64), "labels": torch.tensor([0, 1])}
    with pytest.raises(RuntimeError, match="MI355X only"):
        ClassificationLit(DNAConvNet(**CFG, trainable=True)).train().training_step(batch)
    with pytest.raises(NotImplementedError, match=r"only the head trains on this engine: freeze_backbone=True"):
        ClassificationLit(DNAConvNet(**CFG)).train().training_step(batch)
    with pytest.raises(NotImplementedError, match=r"only the head trains on this engine: freeze_backbone=True"):
        ClassificationLit(_hyena(freeze_backbone=False, precision="fp32")).training_step(batch)
    net = DNAConvNet(**CFG, trainable=True)
    assert net.trainable and not DNAConvNet(**CFG).trainable and net.dropout == 0.1
    import inspect

    par = inspect.signature(DNAConvNet.__init__).parameters["trainable"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False


def test_cnn_yaml_has_the_reference_optimizer(tmp_path):
    from chimeralm_amd.config import compose, instantiate

    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt", "model=cnn"], output_dir=tmp_path)
    model = instantiate(cfg.model)
    opt = model.optimizer_factory(params=model.net.parameters())
    assert type(opt) is torch.optim.Adam and opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["weight_decay"] == 0.0
    sched = model.scheduler_factory(optimizer=opt)
    assert type(sched) is torch.optim.lr_scheduler.ReduceLROnPlateau and sched.patience == 10 and sched.factor == 0.1
    assert not model.net.trainable


BAD_OPTIONS = [(["--epochs", "0"], "--epochs must be"), (["-b", "1"], "--batch-size must be"), (["-b", "0"], "--batch-size must be"),
               (["--lr", "0"], "--lr must be"), (["--val", "reads.bam"], "not in Parquet format"),
               (["--val", "nowhere.parquet"], "no such file"), (["--ckpt", "nowhere.ckpt"], "no such file")]


@pytest.mark.parametrize("args,said", BAD_OPTIONS)
def test_train_refuses_bad_options(args, said):
    """Refused by the command's own checks (their text), before a model is built or a GPU touched."""
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    res = CliRunner().invoke(app, ["train", str(PARQUET), *args], env={"COLUMNS": "250", "TERM": "dumb"})
    assert res.exit_code == 2, res.output
    assert said in " ".join(res.output.replace("│", " ").split()), res.output


def test_train_refuses_bad_files():
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    for path, said in (("reads.bam", "not in Parquet format"), ("missing.parquet", "no such file")):
        res = CliRunner().invoke(app, ["train", path], env={"COLUMNS": "250", "TERM": "dumb"})
        assert res.exit_code == 2 and said in " ".join(res.output.replace("│", " ").split()), res.output


# ------------------------------------------------------------------------------------------------ fit_cnn on a stub net
class _StubCnn(nn.Module):
    """Logits from the base composition of a read, on CPU tensors; every parameter trains."""

    def __init__(self):
        super().__init__()
        self.number_of_classes, self.trainable = 2, True
        self.fc = nn.Linear(16, 2)
        self.seen, self.order = [], []

    def forward(self, ids, quals=None):
        if self.training:
            self.seen.append(ids.shape[0])
            self.order.append(int(ids.sum()))
        return self.fc(F.one_hot(ids, 16).double().mean(dim=1))


def _stub_model(seed=0):
    from chimeralm_amd.basic_module import ClassificationLit

    torch.manual_seed(seed)
    return ClassificationLit(net=_StubCnn().double(), optimizer=partial(torch.optim.Adam, lr=1e-4, weight_decay=0.0),
                             scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=10))


def _fit(tmp, seed=12345, epochs=2, rows=17):
    from chimeralm_amd import cnntrain

    model = _stub_model()
    steps = []
    opt_factory = model.optimizer_factory

    def counting(params):
        opt = opt_factory(params=params)
        step = opt.step
        opt.step = lambda *a, **k: (steps.append(1), step(*a, **k))[1]
        return opt

    model.optimizer_factory = counting
    hist = cnntrain.fit_cnn(model, (str(PARQUET), 0, rows), (str(PARQUET), 18, 25), tmp, epochs=epochs, batch_size=8, lr=1e-2, seed=seed,
                            device="cpu", metrics_factory=_HostSums)
    return model, hist, len(steps)


def test_fit_cnn_on_a_stub_net(tmp_path):
    from safetensors.torch import load_file

    from chimeralm_amd import fit

    m, h, steps = _fit(tmp_path / "a")
    mb, hb, _ = _fit(tmp_path / "b")
    # 17 reads per epoch = 8 + 8 + 1: a batch is never split, one optimizer step per batch, and the last read, alone, has no batch
    # statistics and is left out
    assert m.net.seen == [8, 8] * 2 and steps == 4
    strip = lambda hist: [{k: v for k, v in r.items() if k != "seconds"} for r in hist]   # noqa: E731
    assert strip(h) == strip(hb) and m.net.order == mb.net.order          # seeded order: repeatable ...
    assert m.net.order[:2] != m.net.order[2:]                              # ... and another one per epoch,
    assert _fit(tmp_path / "c", seed=7)[0].net.order != m.net.order        # and per seed
    lines = (tmp_path / "a" / "metrics.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(fit.METRIC_COLUMNS) and len(lines) == 3 and all(len(ln.split("\t")) == 7 for ln in lines[1:])
    assert h[-1]["val/f1_best"] == max(r["val/f1"] for r in h)
    # the best epoch (ties: the earlier) on disk and in memory
    saved, own = load_file(str(tmp_path / "a" / "model.safetensors")), m.state_dict()
    assert sorted(saved) == sorted(own) == ["net.fc.bias", "net.fc.weight"] and all(torch.equal(saved[k], own[k]) for k in own)
    best = min(i for i, r in enumerate(h) if r["val/f1"] == h[-1]["val/f1_best"])
    one, _, _ = _fit(tmp_path / "d", epochs=best + 1)
    assert all(torch.equal(one.state_dict()[k], own[k]) for k in own)
    with pytest.raises(ValueError, match="batch_size >= 2"):
        from chimeralm_amd import cnntrain

        cnntrain.fit_cnn(_stub_model(), (str(PARQUET), 0, 8), (str(PARQUET), 18, 25), tmp_path / "e", epochs=1, batch_size=1, device="cpu",
                         metrics_factory=_HostSums)
