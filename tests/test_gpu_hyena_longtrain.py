"""The segmented Hyena training core on the MI355X (csrc/hyena_longtrain.hip, `clm_hyena_longtrain_*`, chimeralm_amd/hyenatrain.py):
the op against the fp64 formulas at every segment count and at the edges of a segment, disparate scales row by row, determinism and
independence of the reads, agreement with the one-transform op, refusals, one training step of the whole net at 1 x 8,200 against
fp64 autograd through the oracle, the eval forward after a step, and the `finetune --hyena-long-core` option.

Bound of every comparison (the project's, tests/test_gpu_hyena_train.py): max|engine - fp64| / den <= max(8 x the same error of
`fft_core` evaluated in float32 on the CPU, 32 x 2^-24); den is the tensor's maximum, and for the batch-reduced dk, dD, dsw and dsb
the maximum of the sums of the absolute terms.  CLM_HYENA_LONGTRAIN_PARITY=<file> appends the measured ratios to that file
(profiles/hyena_longtrain_parity.txt is one run).
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
# (B, L): smallest | S = 1 | S = 1 full | S = 1 + lone token | two segments, the second of 2 tokens | two full | lone token after two |
# ragged third | the maximum
OP_CASES = [(1, 1), (2, 700), (1, 8192), (1, 8193), (1, 8194), (2, 16384), (1, 16385), (1, 20000), (2, 32769)]
OUTPUTS = ("c", "y") + R.CORE_GRADS


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def _record(rows):
    print("\n".join(rows))
    if os.environ.get("CLM_HYENA_LONGTRAIN_PARITY"):
        with open(os.environ["CLM_HYENA_LONGTRAIN_PARITY"], "a") as f:
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


def _run_core(args, op="long"):
    """The op, forward and backward, on fp32 CPU tensors (zc, sw, sb, k, D, dy) -> its seven outputs (GPU tensors)."""
    from chimeralm_amd import hyenatrain as ht

    fwd, bwd = (ht.long_core_forward, ht.long_core_backward) if op == "long" else (ht.core_forward, ht.core_backward)
    zc, sw, sb, k, D, dy = (t.cuda() for t in args)
    c, y = fwd(zc, sw, sb, k, D)
    grads = bwd(zc, sw, sb, k, D, c, dy)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, (c, y) + tuple(grads)))


def _op(tag, args, ops=("long",)):
    r32 = R.fft_core(*args)
    r64 = R.fft_core(*(t.double() for t in args))
    for op in ops:
        got = _run_core(args, op)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (op, k)
        _check(f"{tag} {op}" if len(ops) > 1 else tag, [(k, got[k], r64[k], r32[k], r64["den"].get(k)) for k in OUTPUTS])


@pytest.mark.parametrize("case", OP_CASES)
def test_long_core_op(case, built_lib):
    B, L = case
    _op(f"long B{B} L{L}", R.random_core(100 + L, B, L))


def test_long_core_op_decaying_filter(built_lib):
    _op("long B1 L16385 decaying k", R.random_core(100 + 16385, 1, 16385, decaying_filter=True))


def test_long_core_op_disparate_scales(built_lib):
    """A training step's magnitudes at two segments, the second of 2 tokens (tests/grad_rows.py `disparate`): through the tensor-wide
    gate, then held per (read, channel) sequence and per channel with the constant of tests/test_gpu_grad_rows.py.  A row that
    misses is a finding about the balancing of the packed sequences, not about the constant."""
    import grad_rows as G

    args, r64, r32 = G.hyena_case(1, 8194, "uniform", "disparate")
    got = {n: t.cpu() for n, t in _run_core(args).items()}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    _check("long B1 L8194 disparate scales", [(k, got[k], r64[k], r32[k], r64["den"].get(k)) for k in OUTPUTS])
    lines, bad = [], []
    G.hold("long B1 L8194 disparate scales", G.hyena_rows(got, r64), G.hyena_rows(r32, r64), G.K["hyena"], lines, bad)
    _record(lines)
    assert not bad, "\n".join(bad)


def test_determinism_and_independence(built_lib):
    """L = 8194, 3 reads.  Two identical calls: identical bits in all seven outputs.  c, y and dzc of read 0: the same bits at
    B = 1, 2 and 3."""
    args = R.random_core(3, 3, 8194)
    a, b = _run_core(args), _run_core(args)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for n in (1, 2):
        zc, sw, sb, k, D, dy = args
        sub = _run_core((zc[:n].contiguous(), sw, sb, k, D, dy[:n].contiguous()))
        for name in ("c", "y", "dzc"):
            assert torch.equal(sub[name][0], a[name][0]), (n, name)


def test_agreement_with_the_one_transform_op(built_lib):
    """At 2 x 700 both ops sit inside the bound against one fp64 reference (no bitwise claim: the transforms differ)."""
    _op("both B2 L700", R.random_core(100 + 700, 2, 700), ops=("long", "one"))


def test_long_core_refusals(built_lib):
    from chimeralm_amd import hyenatrain as ht

    assert ht.MAX_LONG_TOKENS == 32769
    zc, sw, sb, k, D, dy = (t.cuda() for t in R.random_core(1, 1, 32770))
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED: shape or mode outside what the kernels cover"):
        ht.long_core_forward(zc, sw, sb, k, D)
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED"):
        ht.long_core_backward(zc, sw, sb, k, D, torch.zeros_like(dy), dy)
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_UNSUPPORTED"):
        ht.long_workspace_bytes(1, 32770)
    with pytest.raises(ht.HyenaTrainError, match="CLM_E_INVALID"):
        ht.long_workspace_bytes(0, 5)
    zc, sw, sb, k, D, dy = (t.cuda() for t in R.random_core(1, 2, 40))
    c, _ = ht.long_core_forward(zc, sw, sb, k, D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.long_core_forward(zc.double(), sw, sb, k, D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.long_core_forward(zc, sw, sb, k.t().contiguous().t(), D)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.long_core_backward(zc, sw, sb, k, D, c, dy.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ht.long_core_forward(zc.cpu(), sw, sb, k, D)


# ------------------------------------------------------------------------------------------------------------- the net
def _module(sd, trainable=True, hyena_long_core="engine"):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    net = HyenaDna(2, BinarySequenceClassifier(256, dropout=0.0), precision="fp32", selfcheck=False, chunk_reads=4, freeze_backbone=False,
                   trainable=trainable, hyena_core="engine", hyena_long_core=hyena_long_core)
    net.embed_dropout = 0.0
    lit = ClassificationLit(net=net, optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                            scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=10))
    lit.load_state_dict(sd, strict=True)
    return lit.cuda()


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0)


@pytest.fixture(scope="module")
def long_batch():
    return R.step_batch(seed=9, B=1, L=8200, pads=0)


def _step(lit, ids, labels):
    net = lit.net
    seen = {}
    hook = net.head.output_layer.register_forward_hook(lambda m, inp, out: seen.__setitem__("logits", out.detach().cpu()))
    loss = lit.train().training_step({"input_ids": ids.cuda(), "labels": labels.cuda()})
    loss.backward()
    hook.remove()
    return {"loss": loss.detach().cpu(), "logits": seen["logits"], "grads": {k: p.grad.detach().cpu() for k, p in net.named_parameters()}}


def test_long_training_step(sd, long_batch, built_lib):
    """Loss, logits and every p.grad of one training_step at 1 x 8,200 on the segmented op against fp64 autograd through the oracle,
    the float32 oracle as the yardstick; with hyena_long_core="torch" the same batch still ends on the torch core."""
    ids, labels = long_batch
    r64, r32 = R.net_step(sd, ids, labels, torch.float64), R.net_step(sd, ids, labels, torch.float32)
    lit = _module(sd)
    got = _step(lit, ids, labels)
    assert lit.net.last_train_core == "engine-long" and lit.net.hyena_core == "engine"
    assert set(got["grads"]) == set(r64["grads"])
    items = [(k, got[k], r64[k], r32[k], None) for k in ("loss", "logits")]
    items += [(f"d {k}", got["grads"][k], r64["grads"][k], r32["grads"][k], r64["den"].get(k)) for k in sorted(got["grads"])]
    _check("step 1x8200 engine-long", items)
    plain = _module(sd, hyena_long_core="torch")
    _step(plain, ids, labels)
    assert plain.net.last_train_core == "torch"


def test_inference_sees_the_long_step(sd, long_batch, built_lib):
    """After one Adam step at 1 x 8,200 the eval forward moves and equals, bit for bit, a fresh module loaded from the stepped
    state_dict."""
    ids, labels = long_batch
    b = {"input_ids": ids.cuda(), "labels": labels.cuda()}
    lit = _module(sd)
    with torch.no_grad():
        before = lit.eval()(b["input_ids"]).clone()
    opt = torch.optim.Adam(lit.net.parameters(), lr=1e-3)
    lit.train().training_step(b).backward()
    assert lit.net.last_train_core == "engine-long"
    opt.step()
    with torch.no_grad():
        after = lit.eval()(b["input_ids"])
        stepped = {k: v.detach().cpu() for k, v in lit.state_dict().items()}
        fresh = _module(stepped, trainable=False).eval()(b["input_ids"])
    assert torch.equal(after, fresh) and not torch.equal(after, before)


def test_the_finetune_command_takes_the_option(sd, built_lib, golden_dir, tmp_path):
    """`finetune --train-backbone --hyena-long-core engine` in a child process on the golden reads (all short: the option is accepted
    and harmless; the long path is the tests above)."""
    from chimeralm_amd import fit

    start = fit.save_checkpoint(_module(sd), tmp_path / "start")
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "finetune", str(golden_dir / "tests.parquet"), "-o", str(out), "--epochs", "1",
                        "-b", "4", "--seed", "3", "--precision", "fp32", "--train-backbone", "--hyena-long-core", "engine", "--weights",
                        str(start.parent)], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)},
                       cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "model.safetensors").is_file() and len((out / "metrics.tsv").read_text().splitlines()) == 2
