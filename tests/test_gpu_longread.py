"""Reads longer than the model's context on MI355X (csrc/longread.hip through the clm_longread_* C ABI, chimeralm_amd/longread.py, the
`predict --long-reads tile` and `eval.py +long_reads.mode=tile` routes): the two kernels bit for bit against numpy, the pipeline
with a stub net whose answer is known, the windows' logits against each net's plain forward on batches built on the host, and both
entry points on the reference's BAM.  The kernels copy bytes and pick rows, so device results are compared bit for bit; the one
margin (1e-5) is on gaps recomputed from the seven digits the window table prints."""
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import longread_reference as R
import mamba_reference as mr
from oracle import hyena_oracle as ho
from test_gpu_explain import SMALL_SP, _close, _net
from test_longread_host import BAM, LONG_READS, LONG_WINDOWS, _fixture_lengths

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lr(built_lib):
    from chimeralm_amd.longread import LongReads

    h = LongReads("cuda:0")
    yield h
    h.close()


def _device_batch(ids, extra_stride=0):
    """The batch on the device in rows whose stride is a multiple of 16 (and 0xEE behind the columns)."""
    B, L = ids.shape
    buf = torch.full((B, (L + 15) // 16 * 16 + extra_stride), 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :L] = torch.from_numpy(ids).cuda()
    return buf[:, :L]


def _spans_dev(plan):
    return torch.from_numpy(plan.spans.view(np.int32).reshape(-1, 4).copy()).cuda()


def _run_rows(lr, d_ids, d_spans, s0, rows, width, stride):
    out = torch.full((rows + 1, stride), 0xEE, dtype=torch.uint8, device="cuda")
    lr.rows(d_ids, d_spans, s0, rows, out, width)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: rows
@pytest.mark.parametrize("wb", [15, 16, 17, 100])
@pytest.mark.parametrize("half", [False, True])
def test_rows_bit_equal_numpy(lr, wb, half):
    from chimeralm_amd import longread as LR

    o = wb // 2 if half else 0
    opt = LR.Options(window=wb, overlap=o, max_bases=8 * wb)
    n_bases = [3, wb, wb + 1, 3 * wb + 5, 5 * wb + 11]                          # B = 5: two reads that fit, three that do not
    residues = set()
    for shift in range(16):                                                     # 16 left paddings: every source residue mod 16
        L = max(n_bases) + 1 + shift
        ids = R.make_batch(n_bases, 100 * wb + shift, L)
        plan = LR.build_plan(LR.row_lengths(ids), L, opt)
        L_out, first, spans, _ = R.np_plan(R.np_lengths(ids), L, wb, o, 8 * wb)
        assert plan.L_out == L_out == wb + 1 == plan.C and plan.n_extra == first[-1] >= 3
        want = R.np_rows(ids, spans, wb + 1)
        n, width = len(spans), wb + 1
        w16 = (width + 15) // 16 * 16
        stride = w16 + 32                                                        # a row stride beyond the 16-byte rounding
        d_ids, d_spans = _device_batch(ids, extra_stride=16 * (shift % 2)), _spans_dev(plan)
        residues |= {(int(s["src_col"]) - (width - int(s["n_copy"]) - int(s["flags"]))) % 16 for s in plan.spans}
        for s0, rows in ((0, n), (0, 3), (3, n - 4), (n - 1, 1)):               # ragged splits, one across the head / extra boundary
            got = _run_rows(lr, d_ids, d_spans, s0, rows, width, stride)
            assert np.array_equal(got[:rows, :width], want[s0: s0 + rows]), (wb, o, shift, s0, rows)
            assert (got[:rows, width:w16] == 0).all() and (got[:rows, w16:] == 0xEE).all()
            assert (got[rows] == 0xEE).all()                                     # nothing beyond the rows asked for
    assert residues == set(range(16))


def test_rows_at_the_products_size(lr):
    from chimeralm_amd import longread as LR

    opt = LR.Options()                                                           # 32,768 bases, overlap 4,096
    ids = R.make_batch([137_138], 5)                                             # the fixture's longest read
    plan = LR.build_plan(LR.row_lengths(ids), ids.shape[1], opt)
    L_out, first, spans, starts = R.np_plan([137_139], 137_139, 32768, 4096, 262144)
    assert plan.n_windows.tolist() == [5] and plan.starts.tolist() == starts.tolist() == [0, 28672, 57344, 86016, 104370]
    want = R.np_rows(ids, spans, 32769)
    got = _run_rows(lr, _device_batch(ids), _spans_dev(plan), 0, 5, 32769, 32784)
    assert np.array_equal(got[:5, :32769], want) and (got[:5, 32769:] == 0).all() and (got[5] == 0xEE).all()
    assert (got[:5, 32768] == R.SEP).all() and (got[:5, :32768] != R.PAD).all()


def test_rows_refuses_bad_arguments(lr):
    from chimeralm_amd import longread as LR

    ids = R.make_batch([3, 40], 1)
    plan = LR.build_plan(LR.row_lengths(ids), 41, LR.Options(window=16, overlap=0, max_bases=64))
    n = len(plan.spans)
    d_ids, d_spans = _device_batch(ids), _spans_dev(plan)
    out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    flat = torch.full((n * 32 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    odd_ids = torch.zeros((2, 48 + 8), dtype=torch.uint8, device="cuda")[:, :41]
    cases = {
        "misaligned out": lambda: lr.rows(d_ids, d_spans, 0, n, flat[1: 1 + n * 32].view(n, 32), 17),
        "out stride": lambda: lr.rows(d_ids, d_spans, 0, n, torch.zeros((n, 40), dtype=torch.uint8, device="cuda"), 17),
        "out stride below the rounded width": lambda: lr.rows(d_ids, d_spans, 0, n, torch.zeros((n, 16), dtype=torch.uint8, device="cuda"), 17),
        "source stride": lambda: lr.rows(odd_ids, d_spans, 0, n, out, 17),
        "rows > 65535": lambda: lr.rows(d_ids, d_spans, 0, 65536, out, 17),
        "s0 + rows > n_spans": lambda: lr.rows(d_ids, d_spans, 2, n - 1, out, 17),
        "s0 < 0": lambda: lr.rows(d_ids, d_spans, -1, 1, out, 17),
        "no rows": lambda: lr.rows(d_ids, d_spans, 0, 0, out, 17),
    }
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert (out == 0xEE).all() and (flat == 0xEE).all(), "a refused call launched"
    lr.rows(d_ids, d_spans, 0, n, out, 17)                                       # the same arguments, in order
    assert np.array_equal(out.cpu().numpy()[:, :17], R.np_rows(ids, [tuple(s) for s in plan.spans.tolist()], 17))


# ------------------------------------------------------------------------------------------------ 2: reduce
def _reduce(lr, logits, first, B):
    d = torch.from_numpy(logits).cuda()
    n = logits.shape[0]
    out = torch.full((B, 2), 77.0, dtype=torch.float32, device="cuda")
    chosen = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    gap = torch.full((n,), 77.0, dtype=torch.float32, device="cuda")
    bad = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    lr.reduce(d, torch.from_numpy(first).cuda(), B, out, chosen, gap, bad)
    return out.cpu().numpy(), chosen.cpu().numpy(), gap.cpu().numpy(), bad.cpu().numpy()


def _reduce_case(B, seed):
    rng = np.random.default_rng(seed)
    K = rng.integers(1, 10, size=B)                                              # 1 to 9 windows per read ...
    K[B // 2] = 300                                                              # ... and one read with 300
    first = np.concatenate([[0], np.cumsum(K - 1)]).astype(np.int32)
    n = B + int(first[-1])
    # few dyadic values: exactly equal gaps everywhere, also between a read's windows
    logits = (rng.integers(-4, 5, size=(n, 2)) * 0.25).astype(np.float32)
    return first, logits


@pytest.mark.parametrize("B", [1, 12, 300])
def test_reduce_against_numpy(lr, B):
    first, logits = _reduce_case(B, 10 + B)
    rows_of = lambda r: [r] + list(range(B + first[r], B + first[r + 1]))       # noqa: E731
    variants = {"ties": logits}
    z = logits.copy()                                                            # +0.0 / -0.0: equal gaps of either sign
    z[rows_of(B // 2)[:40]] = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 0.0], [-0.0, -0.0]], dtype=np.float32)[np.arange(40) % 4]
    variants["zeros"] = z
    for name, bad_value in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        v = logits.copy()
        for r in range(0, B, 3):                                                 # in either class, in any window, twice in the long read
            rows = rows_of(r)
            v[rows[(r + 1) % len(rows)], r % 2] = bad_value
        v[rows_of(B // 2)[200], 1] = bad_value
        v[rows_of(B // 2)[7], 0] = bad_value
        variants[name] = v
    for name, v in variants.items():
        got = _reduce(lr, v, first, B)
        want = R.np_reduce(v, first, B)
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), name     # the chosen rows, bit for bit
        assert np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[2], want[2], equal_nan=True), name
        assert np.array_equal(got[3], want[3]), name
        rows = [rows_of(r)[got[1][r]] for r in range(B)]
        assert np.array_equal(got[0].view(np.int32), v[rows].view(np.int32)), name
        again = _reduce(lr, v, first, B)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again)), name   # bitwise, run to run
    got = _reduce(lr, variants["nan"], first, B)
    assert got[3][B // 2] >= 2 and got[1][B // 2] == min(k for k, i in enumerate(rows_of(B // 2))
                                                         if not np.isfinite(variants["nan"][i]).all())
    if B > 1:                                                                    # no non-finite window: label = OR of the windows' labels
        got = _reduce(lr, logits, first, B)
        for r in range(B):
            assert (got[0][r, 1] > got[0][r, 0]) == any(logits[i, 1] > logits[i, 0] for i in rows_of(r))


# ------------------------------------------------------------------------------------------------ 3: a stub net with a known answer
class _Counting:
    def __init__(self, net):
        self.net, self.calls = net, []

    def __call__(self, ids, second=None):
        self.calls.append(tuple(ids.shape))
        return self.net(ids, second)


def _stub(ids, second=None):
    """logit1 = the number of N tokens in the row, logit0 = 0.5 (a device function)."""
    n = (ids == 11).sum(1).to(torch.float32)
    return torch.stack([torch.full_like(n, 0.5), n], dim=1).contiguous()


def _np_stub(rows):
    n = (rows == 11).sum(1).astype(np.float32)
    return np.stack([np.full_like(n, 0.5), n], axis=1)


def test_stub_net_pipeline(built_lib):
    from chimeralm_amd import longread as LR

    wb, o = 64, 8
    opt = LR.Options(window=wb, overlap=o, max_bases=1024)
    n_bases = [40, 64, 65, 200, 401]
    ids = R.make_batch(n_bases, 21)
    L = ids.shape[1]

    def plant(r, at, n):
        ids[r, L - 1 - n_bases[r] + at: L - 1 - n_bases[r] + at + n] = 11

    plant(0, 10, 1)                      # a short read with one N: label 1 with or without tiling
    plant(3, 150, 10)                    # behind window 0; windows 2 (112 ... 176) and 3 (136 ... 200) both hold all ten: the lower wins
    plant(4, 300, 3)                     # only in window 5 (280 ... 344)
    net = _Counting(_stub)
    got = LR.tiled_forward(net, _device_batch(ids), options=opt, batch_size=4, lengths=LR.row_lengths(ids))
    assert got.plan.n_windows.tolist() == [1, 1, 2, 4, 8] and got.plan.n_extra == 11
    assert net.calls == [(5, 65), (4, 65), (4, 65), (3, 65)]                     # the head batch whole, then chunks of 4; the last ragged
    torch.cuda.synchronize()
    L_out, first, spans, starts = R.np_plan(R.np_lengths(ids), L, wb, o, 1024)
    window_logits = _np_stub(R.np_rows(ids, spans, 65))
    want = R.np_reduce(window_logits, first, 5)
    assert np.array_equal(got.window_logits.cpu().numpy(), window_logits)
    assert np.array_equal(got.logits.cpu().numpy(), want[0]) and np.array_equal(got.chosen.cpu().numpy(), want[1])
    assert np.array_equal(got.gap.cpu().numpy(), want[2]) and np.array_equal(got.nonfinite.cpu().numpy(), want[3])
    assert want[1].tolist() == [0, 0, 0, 2, 5]
    head_labels = (window_logits[:5, 1] > window_logits[:5, 0]).astype(int).tolist()
    labels = (want[0][:, 1] > want[0][:, 0]).astype(int).tolist()
    assert head_labels == [1, 0, 0, 0, 0] and labels == [1, 0, 0, 1, 1]          # truncated: 0; tiled: 1
    # the window table of the writer
    from chimeralm_amd.callbacks import WindowWriter
    from chimeralm_amd.tokenizer import pack_read_name

    host = got.to_host()
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    names = [f"read{r}" for r in range(5)]
    packed = torch.from_numpy((np.asarray([pack_read_name(n) for n in names], dtype=np.int64) & 0xFF).astype(np.uint8).view(np.int8))
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        WindowWriter(td).write_on_batch_end(SimpleNamespace(global_rank=0), host, {"id": packed}, 0)
        lines = [ln.split("\t") for ln in (Path(td) / "0_0.windows.tsv").read_text().splitlines()]
    assert [ln[0] for ln in lines] == ["read2", "read3", "read4"]
    for ln, r in zip(lines, (2, 3, 4)):
        st = R.window_starts(n_bases[r], wb, o)
        rows = [r] + list(range(5 + first[r], 5 + first[r + 1]))
        assert (int(ln[1]), int(ln[2]), int(ln[3]), ln[5]) == (n_bases[r], len(st), want[1][r], "0")
        assert ln[4] == ";".join(f"{s}:{s + wb}:0.5:{window_logits[i, 1]:.7g}" for s, i in zip(st, rows))


# ------------------------------------------------------------------------------------------------ 4: the five nets
NET_BASES = [100, 256, 257, 700, 1500]


@pytest.mark.parametrize("name", ["hyena", "transformer", "cnn", "mamba", "mambasp"])
def test_windows_equal_plain_forward_on_host_built_batches(built_lib, name):
    from chimeralm_amd import longread as LR

    wb, o, bs = 256, 32, 4
    opt = LR.Options(window=wb, overlap=o, max_bases=4096)
    ids = R.make_batch(NET_BASES, 77)
    L_out, first, spans, _ = R.np_plan(R.np_lengths(ids), ids.shape[1], wb, o, 4096)
    rows = R.np_rows(ids, spans, wb + 1)
    assert first.tolist() == [0, 0, 0, 1, 3, 9]
    batches = [rows[:5]] + [rows[5 + e: 5 + min(e + bs, 9)] for e in range(0, 9, bs)]     # 5, 4, 4, 1 rows
    net = _net(name)
    try:
        got = LR.tiled_forward(net, _device_batch(ids), options=opt, batch_size=bs, lengths=LR.row_lengths(ids))
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in got.tensors().items()}
        plain = np.concatenate([net(torch.from_numpy(b).cuda(), None).cpu().numpy() for b in batches])
        assert g["window_logits"].shape == (14, 2) and np.array_equal(g["window_logits"].view(np.int32), plain.view(np.int32)), name
        want = R.np_reduce(plain, first, 5)
        assert np.array_equal(g["logits"].view(np.int32), want[0].view(np.int32)) and np.array_equal(g["chosen"], want[1])
        assert np.array_equal(g["gap"], want[2]) and np.array_equal(g["nonfinite"], want[3]) and not g["nonfinite"].any()
        again = LR.tiled_forward(net, _device_batch(ids), options=opt, batch_size=bs)      # lengths found from the device batch
        torch.cuda.synchronize()
        assert all(np.array_equal(g[k].view(np.int32), v.cpu().numpy().view(np.int32)) for k, v in again.tensors().items())
    finally:
        _close(net)


def test_no_long_read_in_the_batch(built_lib):
    from chimeralm_amd import longread as LR

    ids = R.make_batch([100, 256, 31], 9)
    net = _net("mambasp")
    try:
        counting = _Counting(net)
        d_ids = _device_batch(ids)
        got = LR.tiled_forward(counting, d_ids, options=LR.Options(window=256, overlap=32, max_bases=4096), batch_size=4,
                               lengths=LR.row_lengths(ids))
        assert counting.calls == [(3, 257)]                                      # once, the batch as it is
        assert got.logits is got.window_logits and got.chosen is None and got.plan.n_extra == 0
        plain = net(d_ids, None)
        torch.cuda.synchronize()
        assert np.array_equal(got.logits.cpu().numpy().view(np.int32), plain.cpu().numpy().view(np.int32))
    finally:
        _close(net)


# ------------------------------------------------------------------------------------------------ 5: predict on the reference's BAM
def _dir_bytes(d):
    return {p.name: p.read_bytes() for p in sorted(Path(d).iterdir())}


@pytest.fixture(scope="module")
def fixture_runs(built_lib, golden_dir, tmp_path_factory):
    """The whole fixture through both feeders, truncating and tiled, with one seeded Hyena model: {(feeder, mode): directory}."""
    from chimeralm_amd import bam, longread as LR, predict as loop, tokenizer as T
    from chimeralm_amd.callbacks import PredictionWriter
    from chimeralm_amd.feeder import BamFeeder
    from chimeralm_amd import lm

    device = torch.device("cuda", 0)
    model = lm.ChimeraLM.new(precision="fp16x3", selfcheck=False)
    model.load_state_dict(ho.make_state_dict(0, head_scale=3.0), strict=True)
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    root = tmp_path_factory.mktemp("longread_predict")
    out = {}
    try:
        for mode in ("truncate", "tile"):
            opt = LR.Options() if mode == "tile" else None
            max_tokens = tok.max_len_single_sentence if opt is None else opt.max_tokens
            d = root / f"native_{mode}"
            with BamFeeder(golden_dir / BAM, batch_size=12, max_tokens=max_tokens) as fd:
                assert loop.run_predict_native(model, fd, PredictionWriter(d), device, long_reads=opt) == 100
                assert fd.stats()["truncated_bases"] == (282_786 if opt is None else 0)
            out["native", mode] = d
            d = root / f"python_{mode}"
            dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / BAM, batch_size=12,
                                   max_length=None if opt is None else opt.max_tokens)
            dm.setup("predict")
            assert loop.run_predict(model, dm, PredictionWriter(d), device, long_reads=opt) == 100
            out["python", mode] = d
    finally:
        _close(model.net)
    return out


def _lines(d):
    files = sorted(Path(d).glob("*.txt"), key=lambda p: int(p.stem.split("_")[1]))
    return [ln.split("\t") for f in files for ln in f.read_text().splitlines()]


def test_predict_fixture_feeders_write_identical_files(fixture_runs):
    for mode in ("truncate", "tile"):
        a, b = _dir_bytes(fixture_runs["native", mode]), _dir_bytes(fixture_runs["python", mode])
        assert sorted(a) == sorted(b) and a == b, mode
    assert not list(fixture_runs["native", "truncate"].glob("*.windows.tsv"))
    assert len(list(fixture_runs["native", "tile"].glob("*.txt"))) == len(list(fixture_runs["native", "truncate"].glob("*.txt"))) == 9


def test_predict_fixture_tile_against_truncate(fixture_runs, golden_dir):
    cut, tiled = _lines(fixture_runs["native", "truncate"]), _lines(fixture_runs["native", "tile"])
    assert len(cut) == len(tiled) == 100 and [c[0] for c in cut] == [t[0] for t in tiled]
    for i, (c, t) in enumerate(zip(cut, tiled)):
        if i not in LONG_READS:
            assert c == t, i                                                     # the 89 short reads: identical lines
        assert not (c[1] == "1" and t[1] == "0"), i                              # no label goes from 1 to 0
    n_bases = _fixture_lengths(golden_dir)
    rows = []
    for f in sorted(fixture_runs["native", "tile"].glob("*.windows.tsv"), key=lambda p: int(p.name.split("_")[1].split(".")[0])):
        batch = int(f.name.split("_")[1].split(".")[0])
        for ln in f.read_text().splitlines():
            rows.append((batch, ln.split("\t")))
    assert [r[1][0] for r in rows] == [tiled[i][0] for i in LONG_READS]          # exactly the 11 reads, in file order
    for (batch, f), i, k in zip(rows, LONG_READS, LONG_WINDOWS):
        assert batch == i // 12 and (int(f[1]), int(f[2])) == (int(n_bases[i]), k)
        table = [w.split(":") for w in f[4].split(";")]
        starts = R.window_starts(int(n_bases[i]), 32768, 4096)
        assert [(int(w[0]), int(w[1])) for w in table] == [(s, s + 32768) for s in starts] and f[5] == "0"
        l0, l1 = float(table[int(f[3])][2]), float(table[int(f[3])][3])
        assert tiled[i][1] == str(int(l1 > l0))                                  # the chosen window's label is the line's
        gaps = [float(w[3]) - float(w[2]) for w in table]
        assert gaps[int(f[3])] >= max(gaps) - 1e-5                               # (the table prints seven digits of logits below 10)
        assert cut[i][1] == str(int(float(table[0][3]) > float(table[0][2])))    # window 0 is the truncated read


# ------------------------------------------------------------------------------------------------ 6: eval.py, any net
def test_eval_py_mambasp_tiles(built_lib, golden_dir, tmp_path):
    sd = {"net." + k: v for k, v in mr.make_mamba_state_dict("mambasp", 0, **SMALL_SP).items()}
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, str(REPO / "eval.py"), f"ckpt_path={ckpt}", "model=mambasp",
                        f"+data.predict_data_path={golden_dir / BAM}", "+long_reads.mode=tile", "+long_reads.window=1024",
                        "+long_reads.overlap=128", "+long_reads.max_bases=4096", f"hydra.run.dir={out}",
                        "model.net.embedding_dim=256", "model.net.number_of_layers=1", "model.net.d_state=16", "model.net.expand=2"],
                       capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _lines(out / "predicts")
    n_bases = np.minimum(_fixture_lengths(golden_dir), 4096)
    assert len(lines) == 100
    tables = {}
    for f in (out / "predicts").glob("*.windows.tsv"):
        for ln in f.read_text().splitlines():
            c = ln.split("\t")
            tables[c[0]] = c
    n_tiled = 0
    for i, (name, label) in enumerate(lines):
        starts = R.window_starts(int(n_bases[i]), 1024, 128)
        if len(starts) == 1:
            assert name not in tables
            continue
        n_tiled += 1
        c = tables[name]
        table = [w.split(":") for w in c[4].split(";")]
        assert (int(c[1]), int(c[2])) == (int(n_bases[i]), len(starts)) and [int(w[0]) for w in table] == starts
        assert c[5] == "0" and label == str(int(any(float(w[3]) > float(w[2]) for w in table)))      # the OR of the windows' labels
    assert n_tiled == len(tables) >= 50
