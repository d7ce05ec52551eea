"""The mutagenesis scan on MI355X (csrc/explain.hip through the clm_explain_* C ABI, chimeralm_amd/explain.py, the `explain` entry
points): the kernels against numpy, the scan against each net's plain forward, and its differences against float64 arithmetic.

Bound of the float64 comparison: |dgap_engine - dgap_fp64| <= 4 x 1e-4 on every window -- 1e-4 is what the project holds fp16x3 and
the Mamba nets to per logit (test_gpu_parity.TOL["fp16x3"], test_gpu_mamba.TOL) and dgap combines four logits.  So that the bound
cannot hide a failure, at least 90 % of a case's windows must have a reference |dgap| >= 4e-3 (ten times the bound); that is
asserted on the reference before the engine is looked at."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cnn_reference as cr
import mamba_reference as mr
from oracle import hyena_oracle as ho
from oracle import transformer_oracle as to
from explain_reference import brute_force_plan, host_batches, make_read as _read, mutant_rows, np_reduce, np_scores

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
DGAP_TOL = 4 * 1e-4
SIGNAL = 10 * DGAP_TOL


@pytest.fixture(scope="module")
def explainer(built_lib):
    from chimeralm_amd.explain import Explainer

    ex = Explainer("cuda:0")
    yield ex
    ex.close()


# ------------------------------------------------------------------------------------------------ 1: mutant rows
@pytest.mark.parametrize("L", [2, 66, 132, 8193])
@pytest.mark.parametrize("w,s,sub", [(1, 1, "N"), (3, 2, "N"), (5, 3, "N"), (1, 1, "all")])
def test_rows_bit_equal_numpy(explainer, L, w, s, sub):
    from chimeralm_amd import explain as E

    ids = _read(L - 1, 300 + L, with_n=L > 2)
    plan_np, _ = E.build_plan(ids, w, s, sub)
    plan, _ = brute_force_plan(ids, w, s, sub)
    want = mutant_rows(ids, plan, w)
    M = len(plan)
    d_ids = torch.from_numpy(ids).cuda()
    d_plan = torch.from_numpy(plan_np.view(np.int32).reshape(M, 4)).cuda()
    stride = (L + 15) // 16 * 16 + 32                         # a row stride beyond the 16-byte rounding of L
    for m0 in sorted({0, (M - 1) // 64 * 64}):               # the first batch and the last, ragged one
        rows = min(64, M - m0)
        out = torch.full((rows + 1, stride), 0xEE, dtype=torch.uint8, device="cuda")
        explainer.rows(d_ids, w, d_plan, m0, rows, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:rows, :L], want[m0:m0 + rows]), (L, w, s, sub, m0)
        assert (got[:rows, L - 1] == 1).all()                # [SEP] untouched in every row
        assert (got[:rows, L:(L + 15) // 16 * 16] == 0).all() and (got[:rows, (L + 15) // 16 * 16:] == 0xEE).all()
        assert (got[rows] == 0xEE).all()                     # nothing beyond the rows asked for


def test_rows_refuses_bad_arguments(explainer):
    from chimeralm_amd import explain as E

    ids = _read(65, 1)
    plan_np, _ = E.build_plan(ids)
    d_ids, d_plan = torch.from_numpy(ids).cuda(), torch.from_numpy(plan_np.view(np.int32).reshape(-1, 4)).cuda()
    out = torch.zeros((8, 80), dtype=torch.uint8, device="cuda")
    for kw in (dict(m0=60, rows=8), dict(m0=-1, rows=1), dict(m0=0, rows=0)):
        with pytest.raises(ValueError):
            explainer.rows(d_ids, 1, d_plan, kw["m0"], kw["rows"], out)
    with pytest.raises(ValueError):                           # a row stride that is no multiple of 16
        explainer.rows(d_ids, 1, d_plan, 0, 4, torch.zeros((8, 70), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):                           # ... or shorter than the read
        explainer.rows(d_ids, 1, d_plan, 0, 4, torch.zeros((8, 64), dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2: reduce
def _reduce(explainer, d, n_bases, w, s, top_k):
    dd = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).cuda()
    imp = torch.empty(n_bases, dtype=torch.float32, device="cuda")
    pos = torch.full((top_k,), 77, dtype=torch.int32, device="cuda")
    val = torch.full((top_k,), 77.0, dtype=torch.float32, device="cuda")
    explainer.reduce(dd, n_bases, w, s, top_k, imp, pos, val)
    return imp.cpu().numpy(), pos.cpu().numpy(), val.cpu().numpy()


@pytest.mark.parametrize("n_bases", [1, 65, 2049, 32768])
@pytest.mark.parametrize("w,s,S", [(1, 1, 1), (1, 1, 4), (5, 3, 1)])
def test_reduce_against_numpy(explainer, n_bases, w, s, S):
    rng = np.random.default_rng(n_bases + 10 * w + S)
    n_windows = -(-n_bases // s)
    # few distinct magnitudes, both signs: ties everywhere, also across the workgroup's threads and waves
    d = (rng.integers(0, 6, size=(n_windows, S)) * rng.choice([-0.125, 0.125], size=(n_windows, S))).astype(np.float32)
    for top_k in (1, 10, 32):                                 # (32 > n_bases for the one-base read)
        got = _reduce(explainer, d, n_bases, w, s, top_k)
        want = np_reduce(d, n_bases, w, s, top_k)
        for g, x, name in zip(got, want, ("importance", "peak_pos", "peak_val")):
            assert np.array_equal(g, x), (name, n_bases, w, s, S, top_k)
        n = min(top_k, n_bases)
        assert (got[1][n:] == -1).all() and (got[2][n:] == 0).all() and (np.diff(got[2][:n]) <= 0).all()
    again = _reduce(explainer, d, n_bases, w, s, 32)
    assert all(np.array_equal(a, b) for a, b in zip(again, _reduce(explainer, d, n_bases, w, s, 32)))


@pytest.mark.parametrize("n_bases", [65, 32768])
def test_reduce_nan_window_and_all_equal(explainer, n_bases):
    w, s = 3, 2
    n_windows = -(-n_bases // s)
    d = np.full((n_windows, 1), 0.5, dtype=np.float32)       # all equal: the peaks are positions 0, 1, 2, ...
    imp, pos, val = _reduce(explainer, d, n_bases, w, s, 8)
    assert (imp == 0.5).all() and pos.tolist() == list(range(8)) and (val == 0.5).all()
    k = n_windows // 2
    d[k, 0] = np.nan                                          # its bases get NaN importance, the read reports no peaks
    imp, pos, val = _reduce(explainer, d, n_bases, w, s, 8)
    want = np_reduce(d, n_bases, w, s, 8)
    assert np.array_equal(imp, want[0], equal_nan=True) and np.isnan(imp).sum() == min(k * s + w, n_bases) - k * s
    assert (pos == -1).all() and (val == 0).all()


# ------------------------------------------------------------------------------------------------ nets with seeded weights
def _close(net):
    if hasattr(net, "close"):
        net.close()
    elif getattr(net, "_engine", None) is not None:           # HyenaDna: its Engine object
        net._engine.close()


def _hyena(seed, prec):
    from chimeralm_amd import lm

    model = lm.ChimeraLM.new(precision=prec, selfcheck=False)
    model.load_state_dict(ho.make_state_dict(seed, head_scale=3.0), strict=True)
    return model.net


def _mamba(variant, seed, prec, **shape):
    from chimeralm_amd import mamba

    d, nl, ds, ex, mml = mr.VARIANTS[variant]
    d, nl, ds, ex = shape.get("d_model", d), shape.get("n_layers", nl), shape.get("d_state", ds), shape.get("expand", ex)
    if variant == "mamba":
        net = mamba.MambaSequenceClassification(vocab_size=12, embedding_dim=d, number_of_layers=nl, model_max_length=mml, dropout=0.1,
                                                number_of_classes=2, d_state=ds, expand=ex, precision=prec)
    else:
        net = mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=d, number_of_layers=nl, number_of_classes=2, dropout=0.2,
                                                  d_state=ds, expand=ex, precision=prec)
    net.load_state_dict(mr.make_mamba_state_dict(variant, seed, **shape), strict=True)
    return net


def _net(name):
    if name == "hyena":
        return _hyena(0, "fp16x3")
    if name in ("mamba", "mambasp"):
        return _mamba(name, 0, "fp16x3")
    if name == "cnn":
        from chimeralm_amd.cnn import DNAConvNet

        net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                         hidden_dim=512, number_of_classes=2, dropout=0.1, precision="fp16x3")
        net.load_state_dict(cr.make_cnn_state_dict(5), strict=True)
        return net
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=12, precision="fp16x3", selfcheck=False)
    net.load_state_dict(to.make_state_dict(5, to.PRODUCTION, scale=1.0), strict=True)
    return net


def _host(imp):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in imp.tensors().items()}


# ------------------------------------------------------------------------------------------------ 3: the scan against the plain forward
@pytest.mark.parametrize("name", ["hyena", "transformer", "cnn", "mamba", "mambasp"])
def test_scan_equals_plain_forward_on_host_built_batches(built_lib, name):
    from chimeralm_amd import explain as E

    net = _net(name)
    try:
        for n_bases, w, s, batch_size in ((65, 1, 1, 7), (65, 1, 1, 64), (131, 3, 2, 7), (131, 3, 2, 64)):
            ids = _read(n_bases, 40 + n_bases, with_n=True)
            plan, n_windows = brute_force_plan(ids, w, s, "N")
            got = _host(E.position_importance(net, torch.from_numpy(ids), window=w, stride=s, score="gap", batch_size=batch_size))
            plain = np.concatenate([net(torch.from_numpy(b).cuda(), None).cpu().numpy() for b in host_batches(ids, plan, w, batch_size)])
            assert got["logits"].shape == (len(plan) + 1, 2) and np.array_equal(got["logits"], plain), (name, n_bases, batch_size)
            dp1, dgap = np_scores(plain)
            assert got["dp1"].shape == got["dgap"].shape == (n_windows, 1)
            assert np.abs(got["dp1"][:, 0] - dp1).max() <= 1e-6 and np.abs(got["dgap"][:, 0] - dgap).max() <= 1e-6
            assert got["n_nonfinite"][0] == 0
            want = np_reduce(got["dgap"], n_bases, w, s, 10)      # the reduce kernel, on the engine's own differences
            assert np.array_equal(got["importance"], want[0]) and np.array_equal(got["peak_pos"], want[1]) \
                and np.array_equal(got["peak_val"], want[2])
            again = _host(E.position_importance(net, torch.from_numpy(ids), window=w, stride=s, score="gap", batch_size=batch_size))
            assert all(np.array_equal(got[k], again[k]) for k in got), (name, n_bases, batch_size)       # bitwise, run to run
        # the default score is the reference's |dp1|, and a string is tokenised as predict does
        seq = "".join("ACGTN"[i - 7] for i in ids[:-1])
        a = _host(E.position_importance(net, seq))
        b = _host(E.position_importance(net, torch.from_numpy(ids), score="prob"))
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert np.array_equal(a["importance"], np.abs(a["dp1"][:, 0]))
    finally:
        _close(net)


# ------------------------------------------------------------------------------------------------ 4: against float64 arithmetic
def _fp64_logits(kind, sd, rows):
    if kind == "hyena":
        return ho.forward(torch.from_numpy(rows.astype(np.int64)), sd, dt=torch.float64).numpy()
    return mr.mamba_forward_fp64(kind, sd, rows.astype(np.int64), device="cuda").cpu().numpy()


CASES64 = [("hyena", 0), ("hyena", 3), ("mambasp", 0), ("mambasp", 1), ("mamba", 0), ("mamba", 1)]


@pytest.fixture(scope="module")
def fp64_dgap():
    """The float64 differences of every case, computed once: (kind, seed, n_bases) -> (ids, w, s, dgap [n_windows])."""
    out = {}
    for kind, seed in CASES64:
        sd = ho.make_state_dict(seed, head_scale=3.0) if kind == "hyena" else mr.make_mamba_state_dict(kind, seed)
        for n_bases, w, s in ((65, 1, 1), (131, 3, 2)):
            ids = _read(n_bases, 500 + n_bases + seed)
            plan, _ = brute_force_plan(ids, w, s, "N")
            rows = np.concatenate([ids[None, :], mutant_rows(ids, plan, w)])
            out[kind, seed, n_bases] = (ids, w, s, np_scores(_fp64_logits(kind, sd, rows))[1])
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("kind,seed", CASES64)
def test_dgap_against_fp64(built_lib, fp64_dgap, kind, seed, prec):
    from chimeralm_amd import explain as E

    net = _hyena(seed, prec) if kind == "hyena" else _mamba(kind, seed, prec)
    try:
        for n_bases in (65, 131):
            ids, w, s, ref = fp64_dgap[kind, seed, n_bases]
            share = float((np.abs(ref) >= SIGNAL).mean())
            print(f"{kind} seed {seed} {n_bases}/{w}/{s}: reference |dgap| >= {SIGNAL:g} on {100 * share:.0f} % of the windows, "
                  f"median {np.median(np.abs(ref)):.3g}")
            assert share >= 0.9, "the reference's differences are too small for the bound to show anything"
            got = _host(E.position_importance(net, torch.from_numpy(ids), window=w, stride=s, score="gap", batch_size=64))
            err = np.abs(got["dgap"][:, 0].astype(np.float64) - ref)
            print(f"{kind} seed {seed} {prec} {n_bases}/{w}/{s}: max |dgap - fp64| = {err.max():.2e}")
            assert err.max() <= DGAP_TOL, (kind, seed, prec, n_bases)
            assert got["n_nonfinite"][0] == 0
    finally:
        _close(net)


# ------------------------------------------------------------------------------------------------ 5: saturation mutagenesis
def test_all_own_base_column_is_zero(built_lib):
    from chimeralm_amd import explain as E

    net = _mamba("mambasp", 0, "fp16x3")
    try:
        ids = _read(65, 77, with_n=True)
        plan, _ = brute_force_plan(ids, 1, 1, "all")
        n_is_n = int((ids[:-1] == 11).sum())
        M = 3 * (65 - n_is_n) + 4 * n_is_n
        assert n_is_n >= 1 and len(plan) == M
        got = _host(E.position_importance(net, torch.from_numpy(ids), substitute="all", score="gap", batch_size=50))
        assert got["logits"].shape == (M + 1, 2) and got["dgap"].shape == got["dp1"].shape == (65, 4)
        plain = np.concatenate([net(torch.from_numpy(b).cuda(), None).cpu().numpy() for b in host_batches(ids, plan, 1, 50)])
        assert np.array_equal(got["logits"], plain)
        dp1, dgap = np_scores(plain)
        want = np.zeros((65, 4))
        want.reshape(-1)[[slot for _, _, slot in plan]] = dgap
        assert np.abs(got["dgap"] - want).max() <= 1e-6
        for b in range(65):
            for c in range(4):
                if ids[b] == 7 + c:                               # exactly 0.0, sign bit included
                    assert got["dgap"][b, c].tobytes() == got["dp1"][b, c].tobytes() == np.float32(0.0).tobytes()
                else:
                    assert got["dgap"][b, c] != 0.0
        assert np.array_equal(got["importance"], np.abs(got["dgap"]).max(1))
    finally:
        _close(net)


def test_nonfinite_mutants_are_counted(explainer):
    """The scores kernel on crafted logits: a NaN / inf mutant has NaN differences and is counted, over two batches of one read."""
    from chimeralm_amd import explain as E

    ids = _read(9, 5)
    plan_np, n_windows = E.build_plan(ids)
    d_plan = torch.from_numpy(plan_np.view(np.int32).reshape(-1, 4)).cuda()
    logits = np.random.default_rng(3).normal(size=(10, 2)).astype(np.float32)
    logits[2, 0], logits[7, 1] = np.nan, np.inf
    f32 = dict(dtype=torch.float32, device="cuda")
    imp = E.Importance(E.Options(), 9, torch.zeros((10, 2), **f32), torch.full((9, 1), 7.0, **f32), torch.full((9, 1), 7.0, **f32),
                       torch.empty(9, **f32), torch.empty(10, dtype=torch.int32, device="cuda"), torch.empty(10, **f32),
                       torch.full((1,), 99, dtype=torch.int32, device="cuda"))
    d = torch.from_numpy(logits).cuda()
    explainer.scores(d[:4].contiguous(), True, d_plan, 0, imp)
    explainer.scores(d[4:].contiguous(), False, d_plan, 3, imp)
    explainer.reduce(imp.dgap, 9, 1, 1, 10, imp.importance, imp.peak_pos, imp.peak_val)
    got = _host(imp)
    dp1, dgap = np_scores(logits)
    assert np.array_equal(got["logits"], logits, equal_nan=True) and got["n_nonfinite"][0] == 2
    bad = np.array([1, 6])
    assert np.isnan(got["dp1"][bad]).all() and np.isnan(got["dgap"][bad]).all() and np.isnan(got["importance"][bad]).all()
    ok = np.setdiff1d(np.arange(9), bad)
    assert np.abs(got["dgap"][ok, 0] - dgap[ok]).max() <= 1e-6 and np.abs(got["dp1"][ok, 0] - dp1[ok]).max() <= 1e-6
    assert (got["peak_pos"] == -1).all() and (got["peak_val"] == 0).all()


# ------------------------------------------------------------------------------------------------ 6: the entry points
def _names_and_reads(golden_dir, n):
    from chimeralm_amd import bam, tokenizer as T
    from chimeralm_amd.callbacks import _read_names

    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / "test_chimric_reads.bam", batch_size=12, max_predict_samples=n)
    dm.setup("predict")
    batch = next(iter(dm.predict_dataloader()))
    reads = [row[int((row != 4).nonzero()[0]):] for row in batch["input_ids"][:n]]
    return _read_names(batch["id"])[:n], reads


def _check_outputs(out_dir, names, reads, net, **options):
    from chimeralm_amd import explain as E

    lines = (out_dir / "0_explain.tsv").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines] == names and all(len(ln.split("\t")) == 12 for ln in lines)
    assert not list(out_dir.glob("*.txt"))
    for i, (ids, ln) in enumerate(zip(reads, lines)):
        want = _host(E.position_importance(net, ids, **options))
        z = np.load(out_dir / f"0_{i}.explain.npz")
        for k, v in want.items():
            assert np.array_equal(z[k], v, equal_nan=True), (i, k)
        f = ln.split("\t")
        assert int(f[5]) == len(ids) - 1 and (int(f[6]), int(f[7]), f[8], f[9]) == (32, 32, "N", "gap")
        assert f[10].split(";")[0] == f"{want['peak_pos'][0]}:{want['peak_val'][0]:.6g}" and f[11] == "0"


def test_cli_explain_hyena(built_lib, golden_dir, tmp_path):
    from chimeralm_amd import lm

    sd = ho.make_state_dict(0, head_scale=3.0)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "explain", str(golden_dir / "test_chimric_reads.bam"), "-o", str(out),
                        "--max-reads", "2", "--window", "32", "--stride", "32", "--score", "gap", "--values", "--ckpt", str(ckpt)],
                       capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names, reads = _names_and_reads(golden_dir, 2)
    model = lm.ChimeraLM.new(precision="fp16x3").load_reference_checkpoint(ckpt)      # the command's default precision
    try:
        _check_outputs(out, names, reads, model, window=32, stride=32, score="gap")
    finally:
        _close(model.net)


SMALL_SP = dict(d_model=256, n_layers=1, d_state=16, expand=2)


def test_explain_py_mambasp(built_lib, golden_dir, tmp_path):
    """The second read has 32,768 bases (1,024 windows of 32,769 tokens each, scanned here and again in this process): the route is
    what is under test, so `model=mambasp` runs at the smallest shape the engine takes (one layer, d 256, d_state 16, expand 2)."""
    sd = {"net." + k: v for k, v in mr.make_mamba_state_dict("mambasp", 0, **SMALL_SP).items()}
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, str(REPO / "explain.py"), f"ckpt_path={ckpt}", "model=mambasp",
                        f"+data.predict_data_path={golden_dir / 'test_chimric_reads.bam'}", "+explain.window=32", "+explain.stride=32",
                        "+explain.score=gap", "+explain.values=true", "+explain.max_reads=2", f"hydra.run.dir={out}",
                        "model.net.embedding_dim=256", "model.net.number_of_layers=1", "model.net.d_state=16", "model.net.expand=2"],
                       capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names, reads = _names_and_reads(golden_dir, 2)
    net = _mamba("mambasp", 0, "fp16x3", **SMALL_SP)
    try:
        _check_outputs(out / "explain", names, reads, net, window=32, stride=32, score="gap")
    finally:
        _close(net)
