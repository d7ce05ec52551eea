"""Training SequenceCNNTransformer on the MI355X (chimeralm_amd/tftrain.py over csrc/attention_train.hip): one training step against
fp64 autograd, the two attention cores against each other, determinism under dropout, the seeds the core is given, the untouched
inference path, a short fit and the `train --net transformer` command.

Bound of every comparison (the project's, tests/test_gpu_mamba_train.py): max|engine - fp64| / max|fp64| <= max(8 x the same error of
the same module evaluated in float32 on the CPU, 32 x 2^-24).  The gradient of `in_proj_bias` is a sum over all positions of dqkv
whose k third cancels exactly in exact arithmetic (a constant added to every key moves no softmax), and that of `attn_pool.bias` is
exactly 0 for the same reason (the pooling softmax): their denominators are the sums of the absolute terms, as in DESIGN.md 5.12 /
5.13.  CLM_ATTN_TRAIN_PARITY=<file> appends the measured ratios to that file.
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

from oracle import transformer_oracle as to

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
FLOOR = 32 * 2.0 ** -24
CFG = to.Config(max_len=256, num_encoder_layers=2)
KW = dict(vocab_size=12, max_len=256, num_encoder_layers=2)
# (reads, tokens): 33 positions, inside one tile, with left padding | 128 positions from 1,031 tokens (every max-pool floors)
BATCHES = {"2x264": (2, 264, 9), "3x1031": (3, 1031, 0)}
_SD = {}


def _state_dict():
    if not _SD:
        _SD.update(to.make_state_dict(21, CFG))
    return _SD


def _net(dropout=0.0, trainable=True, precision="fp32", attention_core="engine", device="cuda"):
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(dropout=dropout, precision=precision, trainable=trainable, attention_core=attention_core, **KW)
    net.load_state_dict(_state_dict())
    return net.to(device)


def _lit(**kw):
    from chimeralm_amd.basic_module import ClassificationLit

    return ClassificationLit(_net(**kw)).cuda()


def _batch(name):
    B, L, pads = BATCHES[name]
    return to.synthetic_ids(5 + L, B, L, pads), np.arange(B) % 2


def _gpu_batch(name):
    ids, labels = _batch(name)
    return {"input_ids": torch.as_tensor(ids).cuda(), "labels": torch.as_tensor(labels).cuda()}


def _step(lit, batch, seed=None):
    seen = {}
    # (the training forward calls the classifier's layers one by one: the hook sits on the last)
    hook = lit.net.classifier[3].register_forward_hook(lambda m, inp, out: seen.__setitem__("logits", out.detach().cpu()))
    lit.train()
    if seed is not None:
        torch.manual_seed(seed)
        lit.net.dropout_generator = torch.Generator(device="cuda").manual_seed(seed)
    loss = lit.training_step(batch)
    loss.backward()
    hook.remove()
    return {"loss": loss.detach().cpu(), "logits": seen["logits"], "grads": {k: p.grad.detach().cpu() for k, p in lit.net.named_parameters()}}


def _cpu_step(name, dtype):
    """The reference's forward statement (transformer.py:82-100) on the module's own containers on the CPU in `dtype`, through
    autograd; with the denominators of the `in_proj_bias` and `attn_pool.bias` gradients: the sums over positions of |dqkv|, |dscore|."""
    from chimeralm_amd import tftrain

    ids, labels = _batch(name)
    ids, labels = torch.as_tensor(ids), torch.as_tensor(labels)
    net = _net(device="cpu", attention_core="torch").to(dtype).train()
    x = net.embedding(ids)
    x = net.cnn(x.transpose(1, 2)).transpose(1, 2)
    x = net.norm(x + net.pos_encoder.pe[:, : x.size(1), :])
    x = net.transformer_encoder(x)
    score = net.attn_pool(x)
    score.retain_grad()
    w = torch.softmax(score, dim=1)
    logits = net.classifier(torch.sum(w * x, dim=1))
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    res = {"loss": loss.detach(), "logits": logits.detach(), "grads": {k: p.grad.detach().clone() for k, p in net.named_parameters()},
           "den": {"attn_pool.bias": score.grad.abs().sum().reshape(1)}}
    if dtype == torch.float64:
        seen, orig = [], tftrain.torch_core

        def rec(qkv, p):
            qkv.retain_grad()
            seen.append(qkv)
            return orig(qkv, p)

        net.zero_grad()
        tftrain.torch_core = rec
        try:
            again = tftrain.train_forward(net, ids)
            torch.nn.functional.cross_entropy(again, labels).backward()
        finally:
            tftrain.torch_core = orig
        assert float((again.detach() - res["logits"]).abs().max()) <= 1e-12      # the restated forward IS the reference's statement
        for i, t in enumerate(seen):
            res["den"][f"transformer_encoder.layers.{i}.self_attn.in_proj_bias"] = t.grad.abs().sum(dim=(0, 1))
    return res


_REF = {}


def _refs(name):
    if name not in _REF:
        _REF[name] = (_cpu_step(name, torch.float64), _cpu_step(name, torch.float32))
    return _REF[name]


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def _compare(tag, got, other, r64, r32):
    """|got - other| / denominator against the bound from r32 - r64, per tensor: prints every figure, returns the failures."""
    rows, bad = [], []
    names = [("loss", None), ("logits", None)] + [(k, k) for k in sorted(got["grads"])]
    for name, g in names:
        pick = (lambda r: r["grads"][g]) if g else (lambda r: r[name])
        den = r64["den"].get(g) if g else None
        d = (pick(r64) if den is None else den).double().abs().max().clamp_min(1e-300)
        if den is not None:
            d = den.double().clamp_min(1e-300)                         # per element: each bias element has its own sum of terms
        err = float(((pick(got).double() - pick(other).double()).abs() / d).max())
        err32 = float(((pick(r32).double() - pick(r64)).abs() / d).max())
        rows.append(f"{tag:26s} {name:58s} {err:.3e}  cpu-fp32 {err32:.3e}  bound {_bound(err32):.3e}  ratio {err / _bound(err32):.3f}")
        if not (np.isfinite(err) and err <= _bound(err32)):
            bad.append(rows[-1])
    print("\n".join(rows))
    if os.environ.get("CLM_ATTN_TRAIN_PARITY"):
        with open(os.environ["CLM_ATTN_TRAIN_PARITY"], "a") as f:
            f.write("\n".join(rows) + "\n")
    return bad


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_training_step(name, built_lib):
    """Loss, logits and every p.grad of one training_step at dropout 0 against fp64 autograd; then the torch core against the engine's."""
    r64, r32 = _refs(name)
    got = _step(_lit(), _gpu_batch(name))
    assert set(got["grads"]) == set(r64["grads"])
    bad = _compare(f"step {name} engine", got, r64, r64, r32)
    via_torch = _step(_lit(attention_core="torch"), _gpu_batch(name))
    bad += _compare(f"step {name} engine-torch", got, via_torch, r64, r32)
    assert not bad, "\n".join(bad)


def test_determinism_and_seeds_with_dropout(built_lib):
    """Two identically seeded steps on fresh modules at dropout 0.1: identical bits.  The core sees dropout_p 0.1 and a seed of its
    own per layer and per step."""
    from chimeralm_amd.tftrain import AttentionCore

    seen = []
    AttentionCore.recorder = lambda p, seed: seen.append((p, seed))
    try:
        b = _gpu_batch("2x264")
        lit = _lit(dropout=0.1)
        a1 = _step(lit, b, seed=5)
        lit.zero_grad()
        a2 = _step(lit, b)                                            # the next step of the same module: new seeds
        b1 = _step(_lit(dropout=0.1), b, seed=5)
    finally:
        AttentionCore.recorder = None
    plain = _step(_lit(dropout=0.0), b, seed=5)
    assert torch.equal(a1["loss"], b1["loss"]) and torch.equal(a1["logits"], b1["logits"])
    for k in a1["grads"]:
        assert torch.equal(a1["grads"][k], b1["grads"][k]), k
    assert not torch.equal(a1["logits"], plain["logits"]) and not torch.equal(a1["logits"], a2["logits"])
    assert len(seen) == 6 and all(p == pytest.approx(0.1) for p, _ in seen)
    seeds = [s for _, s in seen]
    assert len(set(seeds[:4])) == 4 and seeds[4:] == seeds[:2]         # 2 layers x 2 steps all differ; the reseeded module repeats
    assert all(0 <= s < 1 << 64 for s in seeds)


def test_other_paths_are_the_inference_forward(built_lib):
    """trainable=True in eval(), or in train() under no_grad, and trainable=False in train(): the inference kernels, bit for bit."""
    ids = _gpu_batch("2x264")["input_ids"]
    with torch.no_grad():
        want = _lit(trainable=False).eval()(ids)
    plain = _lit(trainable=False, dropout=0.1).train()(ids)
    lit = _lit(dropout=0.1)
    with torch.no_grad():
        quiet = lit.train()(ids)
    assert not plain.requires_grad and torch.equal(plain, want) and torch.equal(quiet, want) and torch.equal(lit.eval()(ids), want)
    assert lit.train()(ids).requires_grad


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_inference_sees_the_step(precision, built_lib):
    """After opt.step() the eval forward moves and equals, bit for bit, a fresh module loaded from the stepped state_dict."""
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.transformer import SequenceCNNTransformer

    b = _gpu_batch("2x264")
    lit = _lit(precision=precision)
    with torch.no_grad():
        before = lit.eval()(b["input_ids"]).clone()
    opt = torch.optim.Adam(lit.net.parameters(), lr=1e-3)
    lit.train().training_step(b).backward()
    opt.step()
    with torch.no_grad():
        after = lit.eval()(b["input_ids"])
        fresh_net = SequenceCNNTransformer(dropout=0.0, precision=precision, **KW)
        fresh_net.load_state_dict({k: v.detach().cpu() for k, v in lit.net.state_dict().items()})
        fresh = ClassificationLit(fresh_net).cuda().eval()(b["input_ids"])
    assert torch.equal(after, fresh) and not torch.equal(after, before)


# ------------------------------------------------------------------------------------------------------------- loop and command
def _write_reads(path: Path, n: int, seed: int):
    """Labelled synthetic reads of 200-400 bases: label 1 = two halves of different base composition, label 0 = one composition."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    rng = np.random.default_rng(seed)
    ids, seqs, quals = [], [], []
    comps = ([0.55, 0.15, 0.15, 0.15], [0.15, 0.15, 0.15, 0.55])
    for i in range(n):
        label, length = i % 2, int(rng.integers(200, 401))
        first = comps[int(rng.integers(2))]
        second = comps[1 - comps.index(first)] if label else first
        half = length // 2
        s = np.concatenate([rng.choice(4, size=half, p=first), rng.choice(4, size=length - half, p=second)])
        ids.append(f"read{seed}_{i}|{label}")
        seqs.append("".join("ACGT"[k] for k in s))
        quals.append([30] * length)
    pq.write_table(pa.table({"id": pa.array(ids, pa.string()), "seq": pa.array(seqs, pa.string()), "qual": pa.array(quals, pa.list_(pa.int32()))}),
                   str(path))


def test_fit_transformer(built_lib, tmp_path):
    from chimeralm_amd import tftrain
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.transformer import SequenceCNNTransformer

    train, val = tmp_path / "train.parquet", tmp_path / "val.parquet"
    _write_reads(train, 64, 1)
    _write_reads(val, 32, 2)
    torch.manual_seed(0)
    net = SequenceCNNTransformer(dropout=0.0, trainable=True, **KW)
    lit = ClassificationLit(net, optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                            scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=6)).cuda()
    hist = tftrain.fit_transformer(lit, (str(train), 0, 64), (str(val), 0, 32), tmp_path / "fit", epochs=4, batch_size=8, lr=3e-4, seed=12345,
                                   device="cuda:0")
    print([(r["train/loss"], r["val/loss"], r["val/f1"]) for r in hist])
    assert len(hist) == 4 and hist[-1]["train/loss"] < hist[0]["train/loss"]
    assert (tmp_path / "fit" / "model.safetensors").is_file() and (tmp_path / "fit" / "metrics.tsv").is_file()


def test_the_train_command_and_eval_py(built_lib, tmp_path):
    """`train --net transformer` (the config's size) in a fresh child process writes a checkpoint eval.py loads; its logits equal the
    in-memory model's."""
    import eval as ev
    from chimeralm_amd.config import compose, instantiate

    data, out = tmp_path / "train.parquet", tmp_path / "cli"
    _write_reads(data, 24, 3)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "chimeralm_amd", "train", str(data), "-o", str(out), "--epochs", "1",
                        "-b", "4", "--seed", "3", "--net", "transformer"], capture_output=True, text=True,
                       env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=330)
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = out / "model.safetensors"
    assert ckpt.is_file() and len((out / "metrics.tsv").read_text().splitlines()) == 2
    _, objs = ev.main([f"ckpt_path={ckpt}", "model=transformer", "data=fq", f"data.test_data_path={data}", "data.batch_size=4",
                       f"hydra.run.dir={tmp_path / 'run'}"])
    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=unused", "model=transformer"], output_dir=tmp_path / "mem")
    mem = instantiate(cfg.model).load_reference_checkpoint(ckpt).cuda().eval()
    ids = torch.as_tensor(to.synthetic_ids(1, 3, 300)).cuda()
    with torch.no_grad():
        assert torch.equal(objs["model"].cuda().eval()(ids), mem(ids))
