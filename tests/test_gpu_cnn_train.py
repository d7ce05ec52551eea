"""GPU (MI355X): DNAConvNet in training mode -- the training kernels (csrc/cnn_train.hip) through the module: the pooling choice
against the fp64 forward, one training step against the fp64 formulas routed by the engine's choice, determinism, the errors, the
inference forward after an optimizer step, a short fit and the `train` command.

The bound of every comparison: err = max |engine - fp64| / max |fp64| must be <= max(8 x the same error of the formulas evaluated in
float32 on the CPU for the same inputs, 32 x 2^-24) -- tests/test_gpu_headtrain.py's bound and floor (the factor covers the kernels'
nested partial sums against torch's one level, the floor keeps a lucky CPU run from failing the test).

Every tensor is held as a whole here, and the largest case stays below the grid caps of `ct_split`; tests/test_gpu_cnn_train_rows.py
holds the same kernels row by row, under shaped inputs and at the capped grids.

CLM_CNN_TRAIN_PARITY=<file> appends the measured ratios to that file (profiles/cnn_train_parity.txt is one).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cnn_reference as cr
import cnn_train_reference as ctr

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
FLOOR = 32 * 2.0 ** -24
CFG = dict(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4], hidden_dim=512,
           number_of_classes=2, padding_idx=4)
# (seed, B, L, pads): one tile with block 2 at 4 -> 1 | positions past 4 L_out in the statistics | exact ties in a pad prefix, L_1 = 50,
# L_2 = 12, tile halos | several tiles per read | workgroups of the dW kernel own several tiles, thousands of homopolymer ties
CASES = [(0, 2, 64, 0), (1, 3, 67, 0), (2, 3, 203, 17), (3, 4, 1031, 100), (4, 8, 2055, 0)]


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


def rel_err(a, b) -> float:
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _module(sd, dropout=0.0, trainable=True, precision="fp32"):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.cnn import DNAConvNet

    net = DNAConvNet(**CFG, dropout=dropout, precision=precision, trainable=trainable)
    net.load_state_dict(sd)
    return ClassificationLit(net).cuda()


def _step(lit, ids, labels):
    """One training_step + backward; -> everything the comparisons read, on the CPU."""
    net = lit.net
    seen = {}
    hooks = [net.fc[0].register_forward_hook(lambda m, inp, out: seen.__setitem__("pooled", inp[0].detach().cpu())),
             net.fc[4].register_forward_hook(lambda m, inp, out: seen.__setitem__("logits", out.detach().cpu()))]
    lit.train()
    loss = lit.training_step({"input_ids": torch.as_tensor(ids).cuda(), "labels": torch.as_tensor(labels).cuda()})
    loss.backward()
    for h in hooks:
        h.remove()
    eng = net.train_engine(torch.device("cuda", torch.cuda.current_device()))
    out = {"loss": loss.detach().cpu(), "pooled": seen["pooled"], "logits": seen["logits"], "grads": {k: p.grad.detach().cpu() for k, p in net.named_parameters()},
           "running": {k: v.detach().cpu() for k, v in net.named_buffers()},
           "mean": net.last_batch_stats[0].cpu(), "var": net.last_batch_stats[1].cpu(),
           "choice": [eng.debug_fetch(f"choice{i}") for i in range(3)], "z": [eng.debug_fetch(f"z{i}") for i in range(3)],
           "dz": [eng.debug_fetch(f"dz{i}") for i in range(3)],
           "masks": None if net.last_dropout_masks is None else [m.cpu().numpy() for m in net.last_dropout_masks]}
    return out


_cases: dict = {}


def _case(case):
    """Inputs, the free-running fp64 reference (torch's own pooling choice) and the engine's step of one case: computed once, shared,
    never changed."""
    if case not in _cases:
        seed, B, L, pads = case
        sd = cr.make_cnn_state_dict(seed)
        ids, labels = cr.synthetic_ids(seed, B, L, pads), ctr.synthetic_labels(seed, B)
        free64 = ctr.cnn_train_reference(sd, ids, labels, torch.float64)
        got = _step(_module(sd), ids, labels)
        _cases[case] = dict(sd=sd, ids=ids, labels=labels, free64=free64, got=got)
    return _cases[case]


def _routed(c, dtype, got=None, p_drop=0.0):
    got = c["got"] if got is None else got
    m = got["masks"]
    return ctr.cnn_train_reference(c["sd"], c["ids"], c["labels"], dtype, choice=got["choice"], keep=None if m is None else m[:3],
                                   fc_keep=None if m is None else m[3], p_drop=p_drop)


@pytest.mark.parametrize("case", CASES)
def test_pooling_choice(case, built_lib):
    """Where fp64's window has an exact tie, or a gap of at least 1e-5 between its two largest values, the engine's choice equals
    torch's (the lowest index that attains the maximum); the windows where it differs all have a gap below 1e-5 and are at most 0.05 %
    per block.  (The fp64 reference computes block 0 through the table, so identical inputs give identical bits there.)"""
    c = _case(case)
    for i in range(3):
        y = c["free64"]["y"][i]
        B, Lin, _ = y.shape
        Lout = Lin // 4
        top = y[:, :4 * Lout].reshape(B, Lout, 4, 256).topk(2, dim=2).values
        gap = top[:, :, 0] - top[:, :, 1]
        differ = torch.from_numpy(c["got"]["choice"][i]) != c["free64"]["choice"][i]
        ties = int((gap == 0).sum())
        print(f"{case} block {i}: {differ.numel()} windows, {ties} exact ties, {int((gap < 1e-5).sum()) - ties} gaps below 1e-5, {int(differ.sum())} differ")
        assert not bool((differ & ((gap == 0) | (gap >= 1e-5))).any())
        assert float(differ.double().mean()) <= 5e-4


def _compare(c, got, ref64, ref32, tag):
    lines, fails = [], []

    def check(name, g, r64, r32):
        err, bound = rel_err(g, r64), _bound(rel_err(r32, r64))
        lines.append(f"{tag} {name}: err {err:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}")
        if not err <= bound:
            fails.append(lines[-1])
        return bound

    assert all(bool(torch.isfinite(v).all()) for v in got["grads"].values())
    check("loss", got["loss"], ref64["loss"], ref32["loss"])
    check("logits", got["logits"], ref64["logits"], ref32["logits"])
    check("pooled", got["pooled"], ref64["pooled"], ref32["pooled"])
    for i in range(3):
        check(f"z{i}", got["z"][i], ref64["z"][i], ref32["z"][i])
        check(f"batch mean {i}", got["mean"][i], ref64["mean"][i], ref32["mean"][i])
        check(f"batch var {i}", got["var"][i], ref64["var"][i], ref32["var"][i])
        check(f"dz{i}", got["dz"][i], ref64["dz"][i], ref32["dz"][i])
    for k in ref64["running"]:
        if not k.endswith("num_batches_tracked"):
            check(k, got["running"][k], ref64["running"][k], ref32["running"][k])
        else:
            assert int(got["running"][k]) == int(ref64["running"][k]), k
    for k in ctr.PARAM_KEYS:
        if k.endswith("0.bias"):
            continue
        check("d " + k, got["grads"][k], ref64["grads"][k], ref32["grads"][k])
    for i in range(3):          # db_i is 0 in exact arithmetic (BatchNorm follows): held to dbeta_i's bound x max |dbeta_i|
        kb, kbeta = f"conv_blocks.{i}.0.bias", f"conv_blocks.{i}.1.bias"
        bound = _bound(rel_err(ref32["grads"][kbeta], ref64["grads"][kbeta])) * float(ref64["grads"][kbeta].abs().max())
        worst = float(got["grads"][kb].abs().max())
        lines.append(f"{tag} |d {kb}| {worst:.3e}  bound {bound:.3e}")
        if not worst <= bound:
            fails.append(lines[-1])
    # d fc.0.bias = sum_b of the gradient at fc.0's output, likewise 0 in exact arithmetic (fc.1 is a BatchNorm), and torch's own sum:
    # the same bound with the size of what cancels in that sum -- per channel the absolute values of all its terms, in fp64
    # (cnn_train_reference: fc0_bias_terms) -- in the place of max |fp64|, which is 0
    scale = float(ref64["fc0_bias_terms"].max())
    bound = max(8.0 * float(ref32["grads"]["fc.0.bias"].abs().max()), FLOOR * scale)
    worst = float(got["grads"]["fc.0.bias"].abs().max())
    lines.append(f"{tag} |d fc.0.bias| {worst:.3e}  bound {bound:.3e}")
    if not worst <= bound:
        fails.append(lines[-1])
    assert bool((got["grads"]["embedding.weight"][4] == 0).all())          # padding_idx, as nn.Embedding gives
    print("\n".join(lines))
    if os.environ.get("CLM_CNN_TRAIN_PARITY"):
        with open(os.environ["CLM_CNN_TRAIN_PARITY"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", CASES)
def test_step_parity_given_the_choice(case, built_lib):
    """One training_step at dropout 0: loss, pooled, z, dz, every p.grad and the running statistics against the fp64 formulas routed by
    the engine's own pooling choice."""
    c = _case(case)
    same = all(bool((torch.from_numpy(c["got"]["choice"][i]) == c["free64"]["choice"][i]).all()) for i in range(3))
    ref64 = c["free64"] if same else _routed(c, torch.float64)
    _compare(c, c["got"], ref64, _routed(c, torch.float32), f"B={case[1]} L={case[2]} pads={case[3]}")


def test_step_with_dropout_and_determinism(built_lib):
    """dropout 0.1 with the masks the module drew handed to the references; a second identical step on a fresh module gives identical
    bits."""
    c = _case(CASES[2])
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        runs.append(_step(_module(c["sd"], dropout=0.1), c["ids"], c["labels"]))
    got, again = runs
    assert got["masks"] is not None and 0.85 < float(got["masks"][0].mean()) < 0.95
    assert torch.equal(got["loss"], again["loss"]) and all(torch.equal(got["grads"][k], again["grads"][k]) for k in got["grads"])
    assert all(np.array_equal(got["dz"][i], again["dz"][i]) for i in range(3))
    _compare(c, got, _routed(c, torch.float64, got, 0.1), _routed(c, torch.float32, got, 0.1), "dropout 0.1 B=3 L=203 pads=17")


def test_backward_accumulates_with_beta_one(built_lib):
    """beta = 1 adds the gradients to what the 13 buffers hold: preset + the beta = 0 result, bit for bit (one fp32 addition each)."""
    from chimeralm_amd.cnntrain import engine_parameters

    c = _case(CASES[2])
    net = _module(c["sd"]).net
    eng, ids = net.train_engine(torch.device("cuda", torch.cuda.current_device())), torch.as_tensor(c["ids"]).cuda()
    params = [p.detach() for p in engine_parameters(net)]
    dp = torch.randn(3, 256, generator=torch.Generator().manual_seed(1)).cuda()
    plain = eng.backward(eng.forward(ids, params, None, 1.0)[3], dp, params)
    preset = [torch.randn(p.shape, generator=torch.Generator().manual_seed(2 + i)).cuda() for i, p in enumerate(params)]
    added = eng.backward(eng.forward(ids, params, None, 1.0)[3], dp, params, out=[t.clone() for t in preset], beta=1.0)
    assert all(bool(g.abs().max() > 0) for i, g in enumerate(plain) if i % 4 != 2)          # (the conv biases' gradients may be 0)
    for i in range(13):
        assert torch.equal(added[i], preset[i] + plain[i]), i


def test_other_paths_are_the_inference_forward(built_lib):
    """trainable=False in train(), and a trainable net in eval() or under no_grad: the inference kernels, bit for bit."""
    c = _case(CASES[2])
    ids = torch.as_tensor(c["ids"]).cuda()
    with torch.no_grad():
        want = _module(c["sd"], trainable=False).eval()(ids)
    plain = _module(c["sd"], trainable=False).train()(ids)
    lit = _module(c["sd"])
    with torch.no_grad():
        quiet = lit.train()(ids)
    assert not plain.requires_grad and torch.equal(plain, want) and torch.equal(quiet, want) and torch.equal(lit.eval()(ids), want)


def test_errors(built_lib):
    from chimeralm_amd.cnntrain import CnnTrainError, engine_parameters

    c = _case(CASES[1])
    ids, labels = torch.as_tensor(c["ids"]).cuda(), torch.as_tensor(c["labels"]).cuda()
    lit = _module(c["sd"]).train()
    first = lit.training_step({"input_ids": ids, "labels": labels})
    lit.training_step({"input_ids": ids, "labels": labels})
    with pytest.raises(RuntimeError, match="another training forward"):
        first.backward()
    assert all(p.grad is None for p in engine_parameters(lit.net))            # (fc's backward ran before the engine's refused)
    with pytest.raises(ValueError, match="at least 2 reads"):
        lit.training_step({"input_ids": ids[:1], "labels": labels[:1]})
    small = _module(c["sd"]).train()
    small.net.train_workspace_limit = 1 << 20
    with pytest.raises(CnnTrainError, match=r"needs \d+ bytes of workspace, the limit is 1048576 bytes"):
        small.training_step({"input_ids": ids, "labels": labels})
    eng = lit.net.train_engine(ids.device)
    gen = eng.generation()
    with pytest.raises(CnnTrainError, match="at most 65535 reads"):       # refused before anything changes: the generation stays
        eng.forward(torch.full((65536, 64), 7, dtype=torch.int64, device="cuda"), [p.detach() for p in engine_parameters(lit.net)], None, 1.0)
    assert eng.generation() == gen
    with pytest.raises(CnnTrainError, match="no forward is pending|another forward"):
        eng.backward(eng.generation() - 1, torch.zeros(3, 256, device="cuda"), [p.detach() for p in engine_parameters(lit.net)])


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_inference_sees_the_step(precision, built_lib):
    """After opt.step() the eval forward equals, bit for bit, a fresh module loaded from the stepped state_dict."""
    c = _case(CASES[2])
    ids, labels = torch.as_tensor(c["ids"]).cuda(), torch.as_tensor(c["labels"]).cuda()
    lit = _module(c["sd"], precision=precision)
    with torch.no_grad():
        before = lit.eval()(ids).clone()
    opt = torch.optim.Adam(lit.net.parameters(), lr=1e-3)
    lit.train().training_step({"input_ids": ids, "labels": labels}).backward()
    opt.step()
    with torch.no_grad():
        after = lit.eval()(ids)
        fresh = _module({k: v.detach().cpu() for k, v in lit.net.state_dict().items()}, precision=precision, trainable=False).eval()(ids)
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


def test_fit_cnn_eval_py_and_the_command(built_lib, tmp_path):
    import eval as ev
    from chimeralm_amd import cnntrain

    train, val = tmp_path / "train.parquet", tmp_path / "val.parquet"
    _write_reads(train, 64, 1)
    _write_reads(val, 32, 2)
    torch.manual_seed(0)
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.cnn import DNAConvNet
    from functools import partial

    lit = ClassificationLit(DNAConvNet(**CFG, dropout=0.1, trainable=True), optimizer=partial(torch.optim.Adam, lr=1e-4, weight_decay=0.0),
                            scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=10)).cuda()
    hist = cnntrain.fit_cnn(lit, (str(train), 0, 64), (str(val), 0, 32), tmp_path / "a", epochs=3, batch_size=8, lr=1e-3, seed=12345,
                            device="cuda:0")
    print([(r["train/loss"], r["val/loss"], r["val/f1"]) for r in hist])
    assert len(hist) == 3 and hist[2]["train/loss"] < hist[0]["train/loss"]
    ckpt = tmp_path / "a" / "model.safetensors"
    metrics, _ = ev.main([f"ckpt_path={ckpt}", "model=cnn", "data=fq", f"data.test_data_path={val}", "data.batch_size=8",
                          f"hydra.run.dir={tmp_path / 'run'}"])
    assert float(metrics["test/f1"]) == pytest.approx(hist[-1]["val/f1_best"], abs=1e-6)
    # the command does the same in a child process: the loss falls, and eval.py reproduces its best val/f1 from its file
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "train", str(train), "--val", str(val), "-o", str(out), "--epochs", "3", "-b", "8",
                        "--lr", "1e-3", "--seed", "3"], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)},
                       cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split("\t") for ln in (out / "metrics.tsv").read_text().splitlines()]
    cols, rows = lines[0], [dict(zip(lines[0], ln)) for ln in lines[1:]]
    assert len(rows) == 3 and float(rows[2]["train/loss"]) < float(rows[0]["train/loss"])
    print([(r_["train/loss"], r_["val/f1"]) for r_ in rows])
    metrics, _ = ev.main([f"ckpt_path={out / 'model.safetensors'}", "model=cnn", "data=fq", f"data.test_data_path={val}", "data.batch_size=8",
                          f"hydra.run.dir={tmp_path / 'run2'}"])
    assert float(metrics["test/f1"]) == pytest.approx(max(float(r_["val/f1"]) for r_ in rows), abs=1e-6)
