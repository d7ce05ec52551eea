"""Training the Mamba nets on the MI355X engine (chimeralm_amd/mambatrain.py, csrc/mamba_train.hip): the core op against the fp64
formulas, one training step of each net against fp64 autograd, determinism, the untouched inference path, a short fit and the
`train --net` command.

Bound of every comparison (the project's, tests/test_gpu_headtrain.py): max|engine - fp64| / max|fp64| <= max(8 x the same error of
the same formulas evaluated in float32 on the CPU, 32 x 2^-24).  `dA_log`, `d dt_bias` and the `dt` columns of `dzxbcdt` are
differences of large sums: their denominator is the sum of the absolute terms (tests/mamba_train_reference.py).
CLM_MAMBA_TRAIN_PARITY=<file> appends the measured ratios to that file (profiles/mamba_train_parity.txt is one).
"""
from __future__ import annotations

import os
import subprocess
import sys
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch

import mamba_reference as mr
import mamba_train_reference as R

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
FLOOR = 32 * 2.0 ** -24
# (expand, N, B, L) at d_model 256: one token | one short chunk | one full chunk at the register-critical N | one token in the second
# chunk | dS carried over more than two chunks at N = 128 | many 64-row tiles per read, H = 12
OP_CASES = [(1, 16, 1, 1), (1, 16, 2, 63), (1, 128, 2, 64), (2, 64, 3, 65), (1, 128, 2, 200), (3, 32, 2, 1031)]
# decay regimes at L = 200 (dt range, A): nothing decays | exp underflows to 0 inside a chunk
REGIMES = {"flat": ((1e-4, 1e-3), 1.0), "steep": ((1e-3, 2.0), 16.0)}


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_MAMBA_TRAIN_PARITY"):
        with open(os.environ["CLM_MAMBA_TRAIN_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _check(tag, items):
    """items: (name, engine, fp64, fp32-on-CPU, denominator tensor or None).  Prints every figure, then asserts them all."""
    rows, bad = [], []
    for name, got, r64, r32, den in items:
        d = float((r64 if den is None else den).double().abs().max().clamp_min(1e-300))
        err = float((got.double().cpu() - r64).abs().max()) / d
        err32 = float((r32.double() - r64).abs().max()) / d
        rows.append(f"{tag:34s} {name:34s} engine {err:.3e}  cpu-fp32 {err32:.3e}  bound {_bound(err32):.3e}  ratio {err / _bound(err32):.3f}")
        if not (np.isfinite(err) and err <= _bound(err32)):
            bad.append(rows[-1])
    _record(rows)
    assert not bad, "\n".join(bad)


def _run_core(zx, p, dout, dims):
    """The engine's op through autograd -> its outputs under the reference's names (GPU tensors)."""
    from chimeralm_amd.mambatrain import Mamba2Core, MambaTrainEngine

    eng = MambaTrainEngine(torch.device("cuda", torch.cuda.current_device()))
    zg = zx.cuda().requires_grad_(True)
    pg = [p[k].cuda().requires_grad_(True) for k in R.CORE_PARAMS]
    out = Mamba2Core.apply(eng, dims, zg, *pg)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dzxbcdt": zg.grad}
    res.update({k: t.grad for k, t in zip(R.CORE_PARAMS, pg)})
    eng.close()
    return res


def _core_items(got, r64, r32, di, N):
    dt0 = 2 * di + 2 * N
    items = [("out", got["out"], r64["out"], r32["out"], None),
             ("dzxbcdt[z|xBC]", got["dzxbcdt"][..., :dt0], r64["dzxbcdt"][..., :dt0], r32["dzxbcdt"][..., :dt0], None),
             ("dzxbcdt[dt]", got["dzxbcdt"][..., dt0:], r64["dzxbcdt"][..., dt0:], r32["dzxbcdt"][..., dt0:], r64["dzxbcdt_dt_abs"])]
    for k in R.CORE_PARAMS:
        den = {"A_log": r64["A_log_abs"], "dt_bias": r64["dt_bias_abs"]}.get(k)
        items.append((f"d {k}", got[k], r64[k], r32[k], den))
    return items


def _op(seed, expand, N, B, L, dt_range=None, A_value=None):
    zx, p, dout = R.random_core(seed, 256, expand, N, B, L, dt_range=dt_range, A_value=A_value, dtype=torch.float32)
    r32 = R.core_backward(zx, p, dout)
    r64 = R.core_backward(zx.double(), {k: v.double() for k, v in p.items()}, dout.double())
    got = _run_core(zx, p, dout, (256, expand, N))
    return got, r64, r32


@pytest.mark.parametrize("case", OP_CASES)
def test_core_op(case, built_lib):
    expand, N, B, L = case
    got, r64, r32 = _op(100 + L, expand, N, B, L)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    if L == 1:
        assert float(got["A_log"].abs().max()) == 0.0                 # one token: the state never decays, dA is exactly 0
    _check(f"op e{expand} N{N} B{B} L{L}", _core_items(got, r64, r32, expand * 256, N))


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_core_op_decay_regimes(regime, built_lib):
    dt_range, A = REGIMES[regime]
    got, r64, r32 = _op(7, 1, 128, 2, 200, dt_range=dt_range, A_value=A)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    _check(f"op {regime} N128 B2 L200", _core_items(got, r64, r32, 256, 128))


def test_core_refusals(built_lib):
    from chimeralm_amd import _native as N
    from chimeralm_amd.mambatrain import MambaTrainEngine, MambaTrainError

    lib = N.load()
    assert lib.clm_mamba_train_workspace_bytes(0, 5, 256, 1, 16) == N.E_INVALID
    assert lib.clm_mamba_train_workspace_bytes(1, 0, 256, 1, 16) == N.E_INVALID
    assert lib.clm_mamba_train_workspace_bytes(1, 5, 384, 1, 16) == N.E_UNSUPPORTED
    assert lib.clm_mamba_train_workspace_bytes(1, 5, 256, 1, 48) == N.E_UNSUPPORTED
    assert lib.clm_mamba_train_workspace_bytes(1 << 16, 1 << 15, 256, 1, 16) == N.E_UNSUPPORTED      # B L = 2^31
    assert lib.clm_mamba_train_workspace_bytes(2, 65, 256, 1, 16) == 4 * (130 * (512 + 4 + 128) + 4 * (256 + 5 * 288 + 4) + 16)
    eng = MambaTrainEngine(torch.device("cuda", torch.cuda.current_device()))
    zx, p, _ = R.random_core(1, 256, 1, 16, 1, 4, dtype=torch.float32)
    with pytest.raises(MambaTrainError, match="supported shapes"):
        eng.forward(zx.cuda(), [p[k].cuda() for k in R.CORE_PARAMS], 256, 1, 48)
    with pytest.raises(ValueError, match="contiguous fp32"):
        eng.forward(zx.cuda().double(), [p[k].cuda() for k in R.CORE_PARAMS], 256, 1, 16)
    eng.close()


# ------------------------------------------------------------------------------------------------------------- the nets
NETS = {
    # variant: (module kwargs, seed, B, L, pads, masked)
    "mambasp": (dict(embedding_dim=256, number_of_layers=2, d_state=16, expand=1), 3, 3, 203, 17, False),
    "mamba": (dict(embedding_dim=256, number_of_layers=2, d_state=64, expand=2, model_max_length=256), 4, 2, 130, 0, True),
}


def _state_dict(variant):
    kw, seed = NETS[variant][0], NETS[variant][1]
    return mr.make_mamba_state_dict(variant, seed, d_state=kw["d_state"], n_layers=kw["number_of_layers"], d_model=kw["embedding_dim"],
                                    expand=kw["expand"], model_max_length=kw.get("model_max_length"))


def _module(variant, sd, dropout=0.0, trainable=True, precision="fp32"):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.mamba import MambaSequenceClassification, MambaSequenceClassificationSP

    cls = MambaSequenceClassification if variant == "mamba" else MambaSequenceClassificationSP
    net = cls(vocab_size=12, number_of_classes=2, dropout=dropout, precision=precision, trainable=trainable, **NETS[variant][0])
    net.load_state_dict(sd)
    return ClassificationLit(net).cuda()


def _batch(variant):
    _, seed, B, L, pads, masked = NETS[variant]
    ids = mr.synthetic_ids(seed, B, L, pads)
    labels = np.arange(B) % 2
    mask = None
    if masked:
        mask = np.ones((B, L), dtype=np.float32)
        mask[0, :9] = 0.0
        mask[1, 100:] = 0.0
    return ids, labels, mask


def _gpu_batch(variant):
    ids, labels, mask = _batch(variant)
    b = {"input_ids": torch.as_tensor(ids).cuda(), "labels": torch.as_tensor(labels).cuda()}
    if mask is not None:
        b["input_quals"] = torch.as_tensor(mask).cuda()
    return b


def _step(lit, batch, seed=None):
    net = lit.net
    seen = {}
    hook = net.classifier.register_forward_hook(lambda m, inp, out: seen.__setitem__("logits", out.detach().cpu()))
    lit.train()
    if seed is not None:
        torch.manual_seed(seed)
    loss = lit.training_step(batch)
    loss.backward()
    hook.remove()
    return {"loss": loss.detach().cpu(), "logits": seen["logits"], "pooled": net.last_train_pooled.cpu(), "route": net.last_train_route.cpu(),
            "grads": {k: p.grad.detach().cpu() for k, p in net.named_parameters()}}


@pytest.mark.parametrize("variant", sorted(NETS))
def test_training_step(variant, built_lib):
    """Loss, logits, pooled and every p.grad of one training_step against fp64 autograd routed by the run's own max-pool positions."""
    sd = _state_dict(variant)
    ids, labels, mask = _batch(variant)
    got = _step(_module(variant, sd), _gpu_batch(variant))
    r64 = R.net_step(variant, sd, ids, labels, mask, route=got["route"], dtype=torch.float64)
    r32 = R.net_step(variant, sd, ids, labels, mask, route=got["route"], dtype=torch.float32)
    assert set(got["grads"]) == set(r64["grads"])
    items = [(k, got[k], r64[k], r32[k], None) for k in ("loss", "logits", "pooled")]
    items += [(f"d {k}", got["grads"][k], r64["grads"][k], r32["grads"][k], r64["den"].get(k)) for k in sorted(got["grads"])]
    _check(f"step {variant}", items)


def test_determinism_with_dropout(built_lib):
    """Two identical steps on fresh modules, dropout on under one seed: identical bits."""
    sd = _state_dict("mamba")
    a = _step(_module("mamba", sd, dropout=0.1), _gpu_batch("mamba"), seed=5)
    b = _step(_module("mamba", sd, dropout=0.1), _gpu_batch("mamba"), seed=5)
    plain = _step(_module("mamba", sd, dropout=0.0), _gpu_batch("mamba"), seed=5)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["logits"], b["logits"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert not torch.equal(a["logits"], plain["logits"])              # (the dropout was on)


@pytest.mark.parametrize("variant", sorted(NETS))
def test_other_paths_are_the_inference_forward(variant, built_lib):
    """trainable=True in eval(), or in train() under no_grad, and trainable=False in train(): the inference kernels, bit for bit."""
    sd = _state_dict(variant)
    b = _gpu_batch(variant)
    args = (b["input_ids"], b.get("input_quals"))
    with torch.no_grad():
        want = _module(variant, sd, trainable=False).eval()(*args)
    plain = _module(variant, sd, trainable=False, dropout=0.1).train()(*args)
    lit = _module(variant, sd, dropout=0.1)
    with torch.no_grad():
        quiet = lit.train()(*args)
    assert not plain.requires_grad and torch.equal(plain, want) and torch.equal(quiet, want) and torch.equal(lit.eval()(*args), want)
    assert lit.train()(*args).requires_grad


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_inference_sees_the_step(precision, built_lib):
    """After opt.step() the eval forward moves and equals, bit for bit, a fresh module loaded from the stepped state_dict."""
    sd = _state_dict("mambasp")
    b = _gpu_batch("mambasp")
    lit = _module("mambasp", sd, precision=precision)
    with torch.no_grad():
        before = lit.eval()(b["input_ids"]).clone()
    opt = torch.optim.Adam(lit.net.parameters(), lr=1e-3)
    lit.train().training_step(b).backward()
    opt.step()
    with torch.no_grad():
        after = lit.eval()(b["input_ids"])
        fresh = _module("mambasp", {k: v.detach().cpu() for k, v in lit.net.state_dict().items()}, precision=precision,
                        trainable=False).eval()(b["input_ids"])
    assert torch.equal(after, fresh) and not torch.equal(after, before)


# ------------------------------------------------------------------------------------------------------------- loop and command
def test_fit_mamba_on_the_golden_reads(built_lib, golden_dir, tmp_path):
    from chimeralm_amd import fit, mambatrain
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.mamba import MambaSequenceClassificationSP

    torch.manual_seed(0)
    net = MambaSequenceClassificationSP(vocab_size=12, number_of_classes=2, dropout=0.0, trainable=True, **NETS["mambasp"][0])
    lit = ClassificationLit(net, optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                            scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=6)).cuda()
    train_rows, val_rows = fit.split_rows(golden_dir / "tests.parquet", None)
    hist = mambatrain.fit_mamba(lit, train_rows, val_rows, tmp_path / "fit", epochs=4, batch_size=4, lr=1e-3, seed=12345, device="cuda:0")
    print([(r["train/loss"], r["val/loss"], r["val/f1"]) for r in hist])
    assert len(hist) == 4 and hist[-1]["train/loss"] < hist[0]["train/loss"]
    assert (tmp_path / "fit" / "model.safetensors").is_file() and (tmp_path / "fit" / "metrics.tsv").is_file()


def test_the_train_command_and_eval_py(built_lib, golden_dir, tmp_path):
    """`train --net mambasp` (the config's size) writes a checkpoint eval.py loads; its logits equal the in-memory model's."""
    import eval as ev
    from chimeralm_amd.config import compose, instantiate

    data, out = golden_dir / "tests.parquet", tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "train", str(data), "-o", str(out), "--epochs", "1", "-b", "4", "--seed", "3",
                        "--net", "mambasp"], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path),
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = out / "model.safetensors"
    assert ckpt.is_file() and len((out / "metrics.tsv").read_text().splitlines()) == 2
    _, objs = ev.main([f"ckpt_path={ckpt}", "model=mambasp", "data=fq", f"data.test_data_path={data}", "data.batch_size=4",
                       f"hydra.run.dir={tmp_path / 'run'}"])
    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=unused", "model=mambasp"], output_dir=tmp_path / "mem")
    mem = instantiate(cfg.model).load_reference_checkpoint(ckpt).cuda().eval()
    ids = torch.as_tensor(mr.synthetic_ids(1, 3, 300)).cuda()
    with torch.no_grad():
        assert torch.equal(objs["model"].cuda().eval()(ids), mem(ids))
