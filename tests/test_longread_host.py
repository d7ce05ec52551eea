"""Host side of `predict --long-reads tile` (chimeralm_amd/longread.py, csrc/longread_plan.cpp, callbacks.WindowWriter, the command
line): no GPU.  The plan is held to a brute-force walk written from the definitions in include/chimeralm_hip.h, and the head batch
to the batches the truncating feeder delivers."""
import ctypes
import os
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import longread_reference as R

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "chimeralm_amd" / "csrc"
BAM = "test_chimric_reads.bam"
LONG_READS = [1, 14, 45, 49, 52, 54, 62, 65, 69, 90, 92]           # file indices of the fixture's reads beyond 32,768 bases
LONG_WINDOWS = [2, 2, 5, 2, 2, 2, 2, 2, 4, 3, 2]                   # their windows at the defaults: 17 extra rows


def _grid():
    for wb in (1, 2, 15, 16, 17, 64):
        for o in sorted({0, 1, wb // 2}):
            if 2 * o > wb:
                continue
            step = wb - o
            for n in (0, 1, wb - 1, wb, wb + 1, wb + step - 1, wb + step, wb + step + 1, 5 * wb + 3):
                if n >= 0:
                    yield wb, o, n


@pytest.mark.parametrize("capped", [False, True])
def test_plan_matches_brute_force(built_lib, capped):
    from chimeralm_amd import longread as LR

    cases = list(_grid())
    assert len(cases) >= 6 * 2 * 8
    for wb, o, n in cases:
        step = wb - o
        max_bases = 2 * wb + 1 if capped else 5 * wb + 3            # (the cap bites on the longest read only)
        lengths = np.array([2, n + 1, wb + 1, n + 1], dtype=np.int32)
        L = int(lengths.max()) + 3                                  # an over-padded batch
        opt = LR.Options(window=wb, overlap=o, max_bases=max_bases)
        plan = LR.build_plan(lengths, L, opt)
        L_out, first, spans, starts = R.np_plan(lengths, L, wb, o, max_bases)
        assert (plan.L_out, plan.C, plan.B, plan.L) == (L_out, wb + 1, 4, L)
        assert np.array_equal(plan.first, first) and np.array_equal(plan.starts, starts)
        assert [tuple(int(x) for x in s) for s in plan.spans.tolist()] == spans, (wb, o, n, capped)
        m = min(n, max_bases)
        assert plan.n_bases.tolist() == [1, m, wb, m]
        K = 1 if n <= wb else 1 + -(-(m - wb) // step)
        assert plan.n_windows.tolist() == [1, K, 1, K]
        win = plan.windows_of(1)
        assert len(win) == K and win[0] == (1, 0)
        if n > wb:
            at = [s for _, s in win]
            covered = np.zeros(m, dtype=bool)
            for i, s in win:
                assert plan.spans[i]["n_copy"] == wb and plan.spans[i]["flags"] == 1     # exactly Wb bases, then [SEP]
                covered[s: s + wb] = True
            assert covered.all()                                                          # every base of [0, min(n, max_bases))
            assert all(0 < b - a <= step for a, b in zip(at, at[1:]))
            assert at[-1] + wb == m                                                       # the last window ends on the last base
        else:
            assert plan.spans[1]["n_copy"] == n + 1 and plan.spans[1]["flags"] == 0       # the read itself, its own [SEP] included
        # the rows the plan stands for: every one ends in [SEP] and holds no pad behind its first token
        ids = R.make_batch([int(x) - 1 for x in lengths], 7 * wb + n, L)
        rows = R.np_rows(ids, spans[4:], wb + 1)
        assert (rows[:, -1] == R.SEP).all() and (rows != R.PAD).all()
        head = R.np_rows(ids, spans[:4], L_out)
        assert np.array_equal(R.np_lengths(head), np.minimum(lengths, wb + 1))


def _fixture_lengths(golden_dir):
    from chimeralm_amd import bam

    return np.array([len(rec["seq"]) for rec in bam.parse_bam_file(golden_dir / BAM)], dtype=np.int64)


def test_plan_of_the_fixture_at_the_defaults(built_lib, golden_dir):
    from chimeralm_amd import longread as LR

    n = _fixture_lengths(golden_dir)
    assert len(n) == 100 and int(n.sum()) == 1_223_444
    opt = LR.Options()
    assert (opt.mode, opt.window_bases, opt.overlap, opt.max_bases, opt.max_tokens) == ("tile", 32768, 4096, 262144, 262145)
    assert np.flatnonzero(n > opt.window_bases).tolist() == LONG_READS
    assert int((n - opt.window_bases).clip(0).sum()) == 282_786 and (n[LONG_READS].min(), n[LONG_READS].max()) == (34_969, 137_138)
    head_tokens = extra_tokens = 0
    windows = []
    for b0 in range(0, 100, 12):
        lengths = (n[b0: b0 + 12] + 1).astype(np.int32)
        plan = LR.build_plan(lengths, int(lengths.max()), opt)
        windows += plan.n_windows.tolist()
        head_tokens += plan.B * plan.L_out
        extra_tokens += plan.n_extra * plan.C
    assert [windows[i] for i in LONG_READS] == LONG_WINDOWS and sum(windows) == 100 + 17
    assert all(w == 1 for i, w in enumerate(windows) if i not in LONG_READS)
    assert (head_tokens, extra_tokens) == (3_065_368, 557_073)


def test_refusals(built_lib):
    from chimeralm_amd import _native as N, longread as LR

    for kw in (dict(window=4, overlap=3), dict(window=0), dict(window=-2), dict(window=8, max_bases=7), dict(overlap=-1),
               dict(mode="all"), dict(window=1.5), dict(overlap=True), dict(max_bases=100)):
        with pytest.raises(ValueError):
            LR.Options(**kw)
    LR.Options(window=8, overlap=4, max_bases=8)
    assert LR.Options(mode="truncate").mode == "truncate"
    with pytest.raises(ValueError):
        LR.tiled_forward(None, torch.zeros((2, 3), dtype=torch.uint8))          # not on a device: refused before anything runs
    with pytest.raises(ValueError):
        LR.build_plan(np.array([9], np.int32), 8, LR.Options(window=4, overlap=0, max_bases=16))    # more tokens than columns
    with pytest.raises(ValueError):
        LR.build_plan(np.array([0], np.int32), 8, LR.Options(window=4, overlap=0, max_bases=16))
    lib = N.load()
    lengths = np.array([30, 3], dtype=np.int32)
    L_out, n_spans = ctypes.c_int(), ctypes.c_int()

    def plan(wb, o, mb, spans=None, cap=0):
        return lib.clm_longread_plan(ctypes.c_void_p(lengths.ctypes.data), 2, 30, wb, o, mb, ctypes.byref(L_out), None,
                                     None if spans is None else ctypes.c_void_p(spans.ctypes.data), None, cap, ctypes.byref(n_spans))

    assert plan(8, 2, 64) == 0 and (L_out.value, n_spans.value) == (9, 2 + 4)   # the count-only call: 29 bases, step 6 -> 5 windows
    for wb, o, mb in ((8, 5, 64), (0, 0, 64), (8, 2, 7), (8, -1, 64)):
        assert plan(wb, o, mb) == N.E_INVALID
        assert lib.clm_longread_last_error(None)
    spans = np.zeros(6, dtype=LR.SPAN_DTYPE)
    assert plan(8, 2, 64, spans[:5].copy(), 5) == N.E_INVALID and n_spans.value == 6    # capacity too small
    assert b"capacity" in lib.clm_longread_last_error(None)
    assert plan(8, 2, 64, spans, 6) == 0

    # lengths: a search per row with the boundary verified
    ids = R.make_batch([0, 1, 15, 16, 17, 40], 3)
    assert LR.row_lengths(ids).tolist() == [1, 2, 16, 17, 18, 41] == R.np_lengths(ids).tolist()
    wide = np.full((6, 64), 0xEE, dtype=np.uint8)                                # a row stride beyond L
    wide[:, :41] = ids
    assert LR.row_lengths(wide[:, :41]).tolist() == [1, 2, 16, 17, 18, 41]
    pads = ids.copy()
    pads[2] = R.PAD                                                              # a row of pads only
    with pytest.raises(ValueError, match="row 2"):
        LR.row_lengths(pads)
    right = ids.copy()
    right[3] = np.roll(right[3], -5)                                             # tokens, then pads: the boundary is broken
    with pytest.raises(ValueError, match="row 3"):
        LR.row_lengths(right)
    with pytest.raises(ValueError):
        LR.row_lengths(ids.astype(np.int64))


@pytest.mark.parametrize("C", [32769, 1025])
def test_window_0_is_the_truncating_feeders_row(built_lib, golden_dir, C):
    from chimeralm_amd import longread as LR
    from chimeralm_amd.feeder import BamFeeder

    with BamFeeder(golden_dir / BAM, batch_size=12, max_tokens=262145, pinned=False, slots=2) as full, \
            BamFeeder(golden_dir / BAM, batch_size=12, max_tokens=C, pinned=False, slots=2) as cut:
        n = 0
        for (ids, names), (want, want_names) in zip(full, cut, strict=True):
            lengths = LR.row_lengths(ids)
            assert np.array_equal(lengths, R.np_lengths(ids))
            head = R.np_head_batch(ids, C - 1)
            assert head.shape == want.shape and np.array_equal(head, want), n
            plan = LR.build_plan(lengths, ids.shape[1], LR.Options(window=C - 1, overlap=0, max_bases=262144))
            assert np.array_equal(R.np_rows(ids, [tuple(s) for s in plan.spans[: len(ids)].tolist()], plan.L_out), want)
            assert np.array_equal(names, want_names)
            n += len(ids)
        assert n == 100
        assert full.stats()["truncated_bases"] == 0
        if C == 32769:
            assert cut.stats()["truncated_bases"] == 282_786


def test_header_native_and_exports(built_lib):
    from chimeralm_amd import _native as N, build, longread as LR

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    declared = set(re.findall(r"\b(clm_longread_[a-z_]+)\s*\(", header))
    assert declared == {"clm_longread_lengths", "clm_longread_plan", "clm_longread_create", "clm_longread_rows", "clm_longread_reduce",
                        "clm_longread_last_error", "clm_longread_destroy"}
    lib = ctypes.CDLL(str(built_lib))
    for name in declared:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS
    assert {"longread.hip", "longread_plan.cpp"} <= set(build.SOURCES)
    assert LR.SPAN_DTYPE.itemsize == ctypes.sizeof(N.ClmLongreadSpan) == 16
    assert "#define CLM_ABI_VERSION 6" in header and N.ABI_VERSION == 6 and lib.clm_abi_version() == 6
    assert "#include <hip" not in (CSRC / "longread_plan.cpp").read_text() + (CSRC / "longread_plan.h").read_text()   # plain C++


def test_longread_kernels_have_no_scratch(built_lib):
    from chimeralm_amd import build

    blocks = [b for b in build.RESOURCES.read_text().split("Function Name: ")[1:] if "longread" in b.splitlines()[0]]
    names = [b.splitlines()[0] for b in blocks]
    assert len(blocks) == 2 and any("longread_rows_kernel" in n for n in names) and any("longread_reduce_kernel" in n for n in names)
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1) == "0", b.splitlines()[0]


def test_cli_refusals(tmp_path):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    runner = CliRunner()
    bam = str(tmp_path / "reads.bam")
    for args, text in ((["--long-reads", "sometimes"], "--long-reads"),
                       (["--long-reads", "tile", "--save-attention"], "--save-attention"),
                       (["--long-reads", "tile", "--long-window", "1024", "--long-overlap", "513"], "overlap")):
        r = runner.invoke(app, ["predict", bam, *args])
        assert r.exit_code == 2, (args, r.output)
        assert text in r.output, (args, r.output)
    r = runner.invoke(app, ["predict", "--help"], env={"COLUMNS": "200", "TERM": "dumb", "NO_COLOR": "1"})
    assert r.exit_code == 0 and "--long-reads" in r.output and "--long-overlap" in r.output and "--long-max-bases" in r.output
    assert "--long-window" not in r.output                                      # hidden


def test_eval_py_refuses_unknown_long_read_keys():
    import eval as ev

    with pytest.raises(ValueError, match="stride"):
        ev.long_read_options({"long_reads": {"mode": "tile", "stride": 3}})
    with pytest.raises(ValueError):
        ev.long_read_options({"long_reads": {"mode": "tile", "overlap": 600, "window": 1024}})
    assert ev.long_read_options({}) is None and ev.long_read_options({"long_reads": {"mode": "truncate"}}) is None
    opt = ev.long_read_options({"long_reads": {"mode": "tile", "window": 1024, "overlap": 128, "max_bases": 4096}})
    assert (opt.window_bases, opt.overlap, opt.max_bases) == (1024, 128, 4096)


def test_window_writer_bytes(tmp_path):
    from chimeralm_amd import longread as LR
    from chimeralm_amd.callbacks import WindowWriter
    from chimeralm_amd.tokenizer import pack_read_name

    def pack_names(names):
        return torch.from_numpy((np.asarray([pack_read_name(n) for n in names], dtype=np.int64) & 0xFF).astype(np.uint8).view(np.int8))

    lengths = np.array([5, 30, 9, 21], dtype=np.int32)
    opt = LR.Options(window=8, overlap=2, max_bases=64)
    plan = LR.build_plan(lengths, 30, opt)                                       # reads 1 (29 bases) and 3 (20 bases) are long
    assert plan.n_windows.tolist() == [1, 5, 1, 3]
    wl = torch.arange(2 * (4 + 6), dtype=torch.float32).reshape(-1, 2) * 0.25
    wl[4 + 1, 1] = 9.0                                                           # read 1's window 2
    tiled = LR.TiledLogits(plan, wl[:4].clone(), wl, torch.tensor([0, 2, 0, 0], dtype=torch.int32),
                           torch.zeros(10), torch.tensor([0, 0, 0, 1], dtype=torch.int32))
    batch = {"id": pack_names(["a", "read/1", "c", "read/3"])}
    w = WindowWriter(tmp_path)
    w.write_on_batch_end(SimpleNamespace(global_rank=2), tiled, batch, 7)
    want = ("read/1\t29\t5\t2\t0:8:0.5:0.75;6:14:2:2.25;12:20:2.5:9;18:26:3:3.25;21:29:3.5:3.75\t0\n"
            "read/3\t20\t3\t0\t0:8:1.5:1.75;6:14:4:4.25;12:20:4.5:4.75\t1\n")
    assert (tmp_path / "2_7.windows.tsv").read_bytes() == want.encode()
    assert not list(tmp_path.glob("*.txt"))                                      # `filter` globs *.txt
    short = LR.build_plan(np.array([5, 9], dtype=np.int32), 9, opt)
    w.write_on_batch_end(SimpleNamespace(global_rank=2), LR.TiledLogits(short, wl[:2], wl[:2]), {"id": pack_names(["a", "b"])}, 8)
    assert not (tmp_path / "2_8.windows.tsv").exists()                           # a batch without long reads writes no file


def test_bam_datamodule_max_length(golden_dir):
    from chimeralm_amd import bam, tokenizer as T

    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    kw = dict(tokenizer=tok, predict_data_path=golden_dir / BAM, batch_size=12, max_predict_samples=12)
    widths = []
    for max_length in (None, 262145):
        dm = bam.BamDataModule(**kw, max_length=max_length)
        dm.setup("predict")
        widths.append(next(iter(dm.predict_dataloader()))["input_ids"].shape[1])
    assert widths[0] == 32769 and widths[1] == _fixture_lengths(golden_dir)[:12].max() + 1 > 32769
    with pytest.raises(TypeError):
        bam.BamDataModule(tok, None, 12, None, None, golden_dir / BAM, 0, None, None, None, None, 262145)    # keyword-only


def test_sanitizer_program(tmp_path):
    exe = tmp_path / "longread_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{REPO / 'include'}", f"-I{CSRC}", str(CSRC / "longread_plan.cpp"), str(REPO / "tests/sanitize/longread_host.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "longread host driver OK" in r.stdout
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert marker not in r.stderr, r.stderr[-4000:]
