"""Fine-tuning the whole HyenaDna net on the MI355X engine (chimeralm_amd/hyenatrain.py, csrc/hyena_train.hip): the core op against
the fp64 formulas at every transform size and alias case, determinism and independence of the reads, refusals, one training step
against fp64 autograd through the oracle, dropout, the untouched inference path, long reads on the torch core, a short fit and the
`finetune --train-backbone` command.

Bound of every comparison (the project's, tests/test_gpu_mamba_train.py): max|engine - fp64| / den <= max(8 x the same error of the
same formulas evaluated in float32 on the CPU, 32 x 2^-24); den is the tensor's maximum, and for the batch-reduced dk, dD, dsw and
dsb the maximum of the sums of the absolute terms (tests/hyena_train_reference.py).
CLM_HYENA_TRAIN_PARITY=<file> appends the measured ratios to that file (profiles/hyena_train_parity.txt is one).
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

import hyena_train_reference as R
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
FLOOR = 32 * 2.0 ** -24
# (B, L): one token | two | logn 8 with the alias, odd B | logn 9 | logn 10 alias | logn 11 | logn 12 | logn 13 alias | logn 14 without
# and with the alias
OP_CASES = [(1, 1), (2, 2), (3, 129), (2, 130), (2, 513), (2, 700), (2, 1031), (1, 4097), (2, 8000), (2, 8193)]
OUTPUTS = ("c", "y") + R.CORE_GRADS


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_HYENA_TRAIN_PARITY"):
        with open(os.environ["CLM_HYENA_TRAIN_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")


def _check(tag, items):
    """items: (name, engine, fp64, fp32-on-CPU, denominator tensor or None).  Prints every figure, then asserts them all."""
    rows, bad = [], []
    for name, got, r64, r32, den in items:
        d = float((r64 if den is None else den).double().abs().max().clamp_min(1e-300))
        err = float((got.double().cpu() - r64).abs().max()) / d
        err32 = float((r32.double() - r64).abs().max()) / d
        rows.append(f"{tag:28s} {name:62s} engine {err:.3e}  cpu-fp32 {err32:.3e}  bound {_bound(err32):.3e}  ratio {err / _bound(err32):.3f}")
        if not (np.isfinite(err) and err <= _bound(err32)):
            bad.append(rows[-1])
    _record(rows)
    assert not bad, "\n".join(bad)


def _run_core(args):
    """The op, forward and backward, on fp32 CPU tensors (zc, sw, sb, k, D, dy) -> its seven outputs (GPU tensors)."""
    from chimeralm_amd import hyenatrain as ht

    zc, sw, sb, k, D, dy = (t.cuda() for t in args)
    c, y = ht.core_forward(zc, sw, sb, k, D)
    grads = ht.core_backward(zc, sw, sb, k, D, c, dy)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, (c, y) + tuple(grads)))


def _op(tag, args):
    r32 = R.fft_core(*args)
    r64 = R.fft_core(*(t.double() for t in args))
    got = _run_core(args)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    _check(tag, [(k, got[k], r64[k], r32[k], r64["den"].get(k)) for k in OUTPUTS])


@pytest.mark.parametrize("case", OP_CASES)
def test_core_op(case, built_lib):
    B, L = case
    _op(f"op B{B} L{L}", R.random_core(100 + L, B, L))


def test_core_op_decaying_filter(built_lib):
    _op("op B2 L1031 decaying k", R.random_core(7, 2, 1031, decaying_filter=True))


def test_core_op_disparate_scales(built_lib):
    """A training step's magnitudes: dy a million times smaller than the activations, a small filter, and one channel of each
    forward pair a thousand times the other.  The sequences a transform packs are balanced first (csrc/hyena_train.hip); packed as
    they come, the smaller one loses its digits to the larger one's rounding.

    Held per (read, channel) sequence and per channel (tests/grad_rows.py, the bound of tests/test_gpu_grad_rows.py): divided by the
    tensor's maximum, the sequences of the odd channels were held a million times looser than the even ones and the claim above was
    not asserted.  The tensor-wide gate still runs first, unchanged."""
    import grad_rows as G

    args, r64, r32 = G.hyena_case(2, 700, "uniform", "disparate")
    _op("op B2 L700 disparate scales", args)
    got = {n: t.cpu() for n, t in _run_core(args).items()}
    lines, bad = [], []
    G.hold("op B2 L700 disparate scales", G.hyena_rows(got, r64), G.hyena_rows(r32, r64), G.K["hyena"], lines, bad)
    _record(lines)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("L", [129, 700])
def test_determinism_and_independence(L, built_lib):
    """Two identical calls: identical bits in every output.  c, y and dzc of read 0: the same bits at B = 1, 2 and 3."""
    args = R.random_core(3, 3, L)
    a, b = _run_core(args), _run_core(args)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in (1, 2):
        zc, sw, sb, k, D, dy = args
        sub = _run_core((zc[:n].contiguous(), sw, sb, k, D, dy[:n].contiguous()))
        for name in ("c", "y", "dzc"):
            assert torch.equal(sub[name][0], a[name][0]), (n, name)


def test_core_refusals(built_lib):
    from chimeralm_amd import hyenatrain as ht

    zc, sw, sb, k, D, dy = (t.cuda() for t in R.random_core(1, 1, 8194))
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED: shape or mode outside what the kernels cover"):
        ht.core_forward(zc, sw, sb, k, D)
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED"):
        ht.workspace_bytes(1, 8194)
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_INVALID"):
        ht.workspace_bytes(0, 5)
    zc, sw, sb, k, D, dy = (t.cuda() for t in R.random_core(1, 2, 40))
    c, _ = ht.core_forward(zc, sw, sb, k, D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.core_forward(zc.double(), sw, sb, k, D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.core_forward(zc, sw, sb, k.t().contiguous().t(), D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.core_backward(zc, sw, sb, k, D, c, dy.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.core_forward(zc.cpu(), sw, sb, k, D)


# ------------------------------------------------------------------------------------------------------------- the net
def _module(sd, dropout=0.0, trainable=True, precision="fp32", hyena_core="engine", freeze=False):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    net = HyenaDna(2, BinarySequenceClassifier(256, dropout=dropout), precision=precision, selfcheck=False, chunk_reads=4,
                   freeze_backbone=freeze, trainable=trainable, hyena_core=hyena_core)
    net.embed_dropout = dropout
    lit = ClassificationLit(net=net, optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                            scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=10))
    lit.load_state_dict(sd, strict=True)
    return lit.cuda()


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0)


@pytest.fixture(scope="module")
def step_reference(sd):
    ids, labels = R.step_batch()
    return ids, labels, R.net_step(sd, ids, labels, torch.float64), R.net_step(sd, ids, labels, torch.float32)


def _gpu_batch(ids, labels):
    return {"input_ids": ids.cuda(), "labels": labels.cuda()}


def _step(lit, batch, seed=None):
    net = lit.net
    seen = {}
    hook = net.head.output_layer.register_forward_hook(lambda m, inp, out: seen.__setitem__("logits", out.detach().cpu()))
    lit.train()
    if seed is not None:
        torch.manual_seed(seed)                                       # the head's dropouts
        net.dropout_generator = torch.Generator(device="cuda").manual_seed(seed)
    loss = lit.training_step(batch)
    loss.backward()
    hook.remove()
    return {"loss": loss.detach().cpu(), "logits": seen["logits"], "grads": {k: p.grad.detach().cpu() for k, p in net.named_parameters()}}


@pytest.mark.parametrize("core", ["engine", "torch"])
def test_training_step(core, sd, step_reference, built_lib):
    """Loss, logits and every p.grad of one training_step at 3 x 203 against fp64 autograd through the oracle; the torch core on the
    GPU sits within the same bound."""
    ids, labels, r64, r32 = step_reference
    lit = _module(sd, hyena_core=core)
    got = _step(lit, _gpu_batch(ids, labels))
    assert lit.net.last_train_core == core
    assert set(got["grads"]) == set(r64["grads"])
    items = [(k, got[k], r64[k], r32[k], None) for k in ("loss", "logits")]
    items += [(f"d {k}", got["grads"][k], r64["grads"][k], r32["grads"][k], r64["den"].get(k)) for k in sorted(got["grads"])]
    _check(f"step 3x203 {core}", items)
    z = got["grads"]["backbone.backbone.layers.3.mixer.filter_fn.pos_emb.z"]
    assert float(z[:, :203].abs().max()) > 0 and float(z[:, 203:].abs().max()) == 0.0


def test_determinism_with_dropout(sd, step_reference, built_lib):
    """Two identical steps on fresh modules, dropout 0.1 under one seed: identical bits, and not the dropout-0 run's."""
    ids, labels = step_reference[:2]
    a = _step(_module(sd, dropout=0.1), _gpu_batch(ids, labels), seed=5)
    b = _step(_module(sd, dropout=0.1), _gpu_batch(ids, labels), seed=5)
    plain = _step(_module(sd, dropout=0.0), _gpu_batch(ids, labels), seed=5)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["logits"], b["logits"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert not torch.equal(a["logits"], plain["logits"])


def test_other_paths_are_the_inference_forward(sd, step_reference, built_lib):
    """trainable=True in eval(), or in train() under no_grad, and trainable=False in train(): the inference kernels, bit for bit."""
    ids = step_reference[0].cuda()
    with torch.no_grad():
        want = _module(sd, trainable=False).eval()(ids)
    plain = _module(sd, trainable=False, dropout=0.1).train()(ids)
    lit = _module(sd, dropout=0.1)
    with torch.no_grad():
        quiet = lit.train()(ids)
    assert not plain.requires_grad and torch.equal(plain, want) and torch.equal(quiet, want) and torch.equal(lit.eval()(ids), want)
    assert lit.train()(ids).requires_grad
    assert lit.net.last_train_core == "engine"
    frozen = _module(sd, freeze=True)                                # the head fine-tune keeps its own path
    assert frozen.train()(ids).requires_grad and frozen.net.last_train_core is None
    assert all(p.grad is None for p in frozen.net.parameters())


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_inference_sees_the_step(precision, sd, step_reference, built_lib):
    """After one Adam step the eval forward moves and equals, bit for bit, a fresh module loaded from the stepped state_dict (the
    filter spectra included: the filter MLP moved too)."""
    ids, labels = step_reference[:2]
    b = _gpu_batch(ids, labels)
    lit = _module(sd, precision=precision)
    with torch.no_grad():
        before = lit.eval()(b["input_ids"]).clone()
    opt = torch.optim.Adam(lit.net.parameters(), lr=1e-3)
    lit.train().training_step(b).backward()
    opt.step()
    with torch.no_grad():
        after = lit.eval()(b["input_ids"])
        stepped = {k: v.detach().cpu() for k, v in lit.state_dict().items()}
        fresh = _module(stepped, precision=precision, trainable=False).eval()(b["input_ids"])
    assert not torch.equal(stepped["net.backbone.backbone.layers.0.mixer.filter_fn.implicit_filter.2.weight"],
                           sd["net.backbone.backbone.layers.0.mixer.filter_fn.implicit_filter.2.weight"])
    assert torch.equal(after, fresh) and not torch.equal(after, before)


def test_long_reads_take_the_torch_core(sd, built_lib):
    ids, labels = R.step_batch(seed=9, B=1, L=8200, pads=0)
    lit = _module(sd)
    got = _step(lit, _gpu_batch(ids, labels))
    assert lit.net.last_train_core == "torch" and lit.net.hyena_core == "engine"
    assert bool(torch.isfinite(got["loss"]))
    for k, g in got["grads"].items():
        assert bool(torch.isfinite(g).all()), k


# ------------------------------------------------------------------------------------------------------------- loop and command
def test_fit_hyena_on_the_golden_reads(sd, built_lib, golden_dir, tmp_path):
    """4 epochs at batch 4, dropout 0, at the model's own AdamW rate 1e-4 (chosen on the CPU with the torch core, where train/loss
    went 0.733, 0.714, 0.686, 0.696; 3e-4 and 1e-3 fell too, less smoothly)."""
    from chimeralm_amd import fit, hyenatrain

    lit = _module(sd)
    train_rows, val_rows = fit.split_rows(golden_dir / "tests.parquet", None)
    hist = hyenatrain.fit_hyena(lit, train_rows, val_rows, tmp_path / "fit", epochs=4, batch_size=4, lr=1e-4, seed=12345, device="cuda:0")
    print([(r["train/loss"], r["val/loss"], r["val/f1"]) for r in hist])
    assert len(hist) == 4 and hist[-1]["train/loss"] < hist[0]["train/loss"]
    assert lit.net.last_train_core == "engine"
    assert (tmp_path / "fit" / "model.safetensors").is_file() and (tmp_path / "fit" / "metrics.tsv").is_file()


def test_the_finetune_command_and_eval_py(sd, built_lib, golden_dir, tmp_path):
    """`finetune --train-backbone` in a child process from a checkpoint saved here writes a checkpoint eval.py loads; its logits equal
    the in-memory model's."""
    import eval as ev
    from chimeralm_amd import fit, lm

    start = fit.save_checkpoint(_module(sd), tmp_path / "start")
    data, out = golden_dir / "tests.parquet", tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "finetune", str(data), "-o", str(out), "--epochs", "1", "-b", "4", "--seed", "3",
                        "--train-backbone", "--weights", str(start.parent)], capture_output=True, text=True,
                       env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = out / "model.safetensors"
    assert ckpt.is_file() and len((out / "metrics.tsv").read_text().splitlines()) == 2
    from safetensors.torch import load_file

    new = load_file(str(ckpt))
    assert not torch.equal(new["net.backbone.backbone.layers.0.mixer.in_proj.weight"], sd["net.backbone.backbone.layers.0.mixer.in_proj.weight"])
    _, objs = ev.main([f"ckpt_path={ckpt}", "model=hyena", "model.net.precision=fp32", "data=fq", f"data.test_data_path={data}",
                       "data.batch_size=4", f"hydra.run.dir={tmp_path / 'run'}"])
    mem = lm.ChimeraLM.new(precision="fp32", selfcheck=False).load_reference_checkpoint(ckpt).cuda().eval()
    ids = R.step_batch(seed=1, B=3, L=300, pads=20)[0].cuda()
    with torch.no_grad():
        assert torch.equal(objs["model"].cuda().eval()(ids), mem(ids))
