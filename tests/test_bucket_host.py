"""Host side of `predict --batching bucket` (chimeralm_amd/bucket.py, csrc/bucket_plan.cpp, the command line, eval.py): no GPU.  The
canonical length is held to the table and the properties of include/chimeralm_hip.h, the planner to a small Python model written
here from the same definitions, and to the invariants themselves: every read once, rows in arrival order, a class emitted exactly
when full, the end flush in ascending length, no two live rows on the same pool bytes, a scatter group closed at every emit."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "chimeralm_amd" / "csrc"
MAX_TOKENS = 32769
KNOWN = {1: 65, 65: 65, 66: 129, 1025: 1025, 1026: 1153, 8193: 8193, 8194: 9217, 30000: 30721, 32769: 32769}


def model_length(n, m=3):
    """Lc(n) of the header, restated."""
    b = n - 1
    q = 1 << max(6, max(b, 1).bit_length() - 1 - m)
    return min(MAX_TOKENS, 1 + q * max(1, -(-b // q)))


def _round16(n):
    return -(-n // 16) * 16


class ModelPlanner:
    """The regrouping of the header in Python: (kind, ...) tuples in the planner's order."""

    def __init__(self, batch_size, m):
        self.batch_size, self.m, self.classes, self.used, self.count = batch_size, m, {}, 0, 0

    def push(self, lengths, L):
        steps, group = [], []
        for r, n in enumerate(int(x) for x in lengths):
            lc = model_length(n, self.m)
            if lc not in self.classes:
                self.classes[lc] = (self.used, [])
                self.used += _round16(lc) * self.batch_size
            off, reads = self.classes[lc]
            group.append((r, L - n, n, lc, off + len(reads) * _round16(lc)))
            reads.append(self.count)
            self.count += 1
            if len(reads) == self.batch_size:
                steps += [("scatter", group), ("emit", lc, off, _round16(lc), list(reads))]
                group = []
                reads.clear()
        return steps + ([("scatter", group)] if group else [])

    def finish(self):
        steps = []
        for lc in sorted(self.classes):
            off, reads = self.classes[lc]
            if reads:
                steps.append(("emit", lc, off, _round16(lc), list(reads)))
                reads.clear()
        return steps


def _as_tuples(steps, spans, reads):
    from chimeralm_amd import _native as N

    out = []
    for st in steps:
        if st["kind"] == N.BUCKET_SCATTER:
            assert (st["length"], st["offset"], st["stride"]) == (0, 0, 0)
            out.append(("scatter", [tuple(int(x) for x in s) for s in spans[st["first"]: st["first"] + st["count"]].tolist()]))
        else:
            assert st["kind"] == N.BUCKET_EMIT
            out.append(("emit", int(st["length"]), int(st["offset"]), int(st["stride"]),
                        reads[st["first"]: st["first"] + st["count"]].tolist()))
    return out


def _class_tops(m=3):
    tops, n = [], 1
    while n <= MAX_TOKENS:
        tops.append(model_length(n, m))
        n = tops[-1] + 1
    return tops


def _reads(seed=0, m=3):
    """2,000 seeded reads, log-uniform in 1 ... 32,769 tokens, and every ladder edge with its two neighbours."""
    rng = np.random.default_rng(seed)
    n = np.exp(rng.uniform(0.0, np.log(MAX_TOKENS), 2000)).round().astype(np.int64).clip(1, MAX_TOKENS)
    edges = [t + d for t in _class_tops(m) for d in (-1, 0, 1) if 1 <= t + d <= MAX_TOKENS]
    return np.concatenate([n, np.asarray(edges, dtype=np.int64)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the canonical length
def test_canonical_length_table_and_properties(built_lib):
    from chimeralm_amd import bucket as B

    for n, lc in KNOWN.items():
        assert B.canonical_length(n) == lc == model_length(n), n
    lib_lc = np.array([B.canonical_length(n) for n in range(1, MAX_TOKENS + 1)])
    n = np.arange(1, MAX_TOKENS + 1)
    assert np.array_equal(lib_lc, [model_length(int(x)) for x in n])
    assert (lib_lc >= n).all() and (lib_lc >= 65).all() and (np.diff(lib_lc) >= 0).all() and lib_lc.max() == MAX_TOKENS
    pads, bases = lib_lc - n, n - 1
    assert (pads <= np.maximum(64, bases / 8)).all()                                     # at most max(64, b / 8) pads
    assert (pads[n >= 600] / lib_lc[n >= 600]).max() <= 0.1112                           # 11.1 % of a row at the worst from 600 tokens on
    tops = sorted(set(lib_lc.tolist()))
    assert len(tops) == 56 and tops == _class_tops()
    assert {1025, 2049, 4097, 8193, 16385, 32769} <= set(tops)                           # the engine's natural sizes: no pad
    assert all(B.canonical_length(t) == t for t in tops)
    assert all(t <= 1025 or (t - 1) % 64 == 0 for t in tops) and tops[:16] == [65 + 64 * i for i in range(16)]
    assert B.pool_bytes(1) == sum(_round16(t) for t in tops) == 406_400 and B.pool_bytes(256) == 256 * 406_400
    for m in range(6):                                                                   # every allowed steps_log2, at the edges
        opt = B.Options(steps_log2=m)
        for t in _class_tops(m):
            for d in (-1, 0, 1):
                if 1 <= t + d <= MAX_TOKENS:
                    assert B.canonical_length(t + d, opt) == model_length(t + d, m)


def test_fixture_bam_counts(built_lib, golden_dir):
    """The figures of the issue for the reference's test BAM: 39 classes and 963,236 tokens at m = 3, against 3,065,368 in batches
    of 12 in file order."""
    from chimeralm_amd import bam, bucket as B

    n = np.array([min(len(rec["seq"]), 32768) + 1 for rec in bam.parse_bam_file(golden_dir / "test_chimric_reads.bam")])
    lc = np.array([B.canonical_length(int(x)) for x in n])
    assert len(n) == 100 and int(n.sum()) == 940_758 and (n.min(), n.max()) == (525, 32769)
    assert len(set(lc.tolist())) == 39 and int(lc.sum()) == 963_236
    assert sum(len(n[i: i + 12]) * int(n[i: i + 12].max()) for i in range(0, 100, 12)) == 3_065_368


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("batch_size", [1, 3, 256])
@pytest.mark.parametrize("push", [1, 7, 64])
def test_planner_against_the_model_and_the_invariants(built_lib, batch_size, push):
    from chimeralm_amd import bucket as B

    all_reads = _reads()
    assert len(all_reads) > 2000 + 56
    planner, model = B.Planner(batch_size), ModelPlanner(batch_size, 3)
    pool = B.pool_bytes(batch_size)
    emitted, held, live, slabs = [], {}, set(), {}
    count = 0

    def walk(steps, lengths, L, finish):
        nonlocal count
        kinds = [s[0] for s in steps]
        assert all(a != b or a == "emit" for a, b in zip(kinds, kinds[1:])), "two scatter groups with no emit between them"
        if finish:
            assert all(k == "emit" for k in kinds)
            assert [s[1] for s in steps] == sorted(s[1] for s in steps) and len({s[1] for s in steps}) == len(steps)   # ascending Lc
        row = 0
        for i, st in enumerate(steps):
            if st[0] == "scatter":
                for r, col, n, lc, off in st[1]:
                    assert r == row and n == lengths[r] and col == L - n and lc == model_length(n)
                    stride = _round16(lc)
                    base = slabs.setdefault(lc, off)                                 # the class's first read is row 0 of its slab
                    slot = (off - base) // stride
                    assert (off - base) % stride == 0 and slot == len(held.setdefault(lc, [])) < batch_size
                    assert 0 <= off and off + stride <= pool and off not in live
                    live.add(off)
                    held[lc].append(count)
                    count += 1
                    row += 1
            else:
                _, lc, off, stride, reads = st
                assert off == slabs[lc] and stride == _round16(lc) and reads == held[lc]      # arrival order
                assert len(reads) == batch_size if not finish else 1 <= len(reads) <= batch_size
                if not finish:
                    assert steps[i - 1][0] == "scatter" and steps[i - 1][1][-1][3] == lc       # the group closes with the row that fills it
                for k in range(len(reads)):
                    live.remove(off + k * stride)
                emitted.extend(reads)
                held[lc] = []
        if not finish:
            assert row == len(lengths)
            assert all(len(v) < batch_size for v in held.values())                   # a class emits exactly when it is full

    for i in range(0, len(all_reads), push):
        lengths = all_reads[i: i + push]
        L = int(lengths.max()) + (i % 3)                                             # sometimes an over-padded batch
        got = _as_tuples(*planner.push(lengths, L))
        assert got == model.push(lengths, L), (batch_size, push, i)
        walk(got, lengths.tolist(), L, False)
    got = _as_tuples(*planner.finish())
    assert got == model.finish()
    walk(got, [], 0, True)
    assert sorted(emitted) == list(range(len(all_reads))) and not live              # every read exactly once
    spans = sorted((off, off + _round16(lc) * batch_size) for lc, off in slabs.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= pool     # the slabs are disjoint and inside the pool
    assert _as_tuples(*planner.finish()) == []
    planner.close()


def test_refusals_and_option_validation(built_lib):
    from chimeralm_amd import _native as N, bucket as B

    for kw in (dict(mode="length"), dict(steps_log2=-1), dict(steps_log2=6), dict(steps_log2=1.5), dict(steps_log2=True),
               dict(steps_log2="3")):
        with pytest.raises(ValueError):
            B.Options(**kw)
    assert (B.Options().mode, B.Options().steps_log2, B.Options(mode="file").mode) == ("bucket", 3, "file")
    for n in (0, -1, MAX_TOKENS + 1, 2.5):
        with pytest.raises(ValueError):
            B.canonical_length(n)
    for bs in (0, 65536, -3, 1.5):
        with pytest.raises(ValueError):
            B.Planner(bs)
        with pytest.raises(ValueError):
            B.pool_bytes(bs)
    planner = B.Planner(4)
    planner.push([100, 200], 200)
    for lengths, L in (([0], 8), ([9], 8), ([5, MAX_TOKENS + 1], MAX_TOKENS + 1), ([], 8)):
        with pytest.raises(ValueError):
            planner.push(lengths, L)
    steps, spans, reads = planner.finish()                                           # a refused push changed nothing
    assert [int(s["length"]) for s in steps] == [129, 257] and reads.tolist() == [0, 1]
    lib = N.load()
    assert lib.clm_bucket_length(0, 3) == N.E_INVALID and lib.clm_bucket_plan_last_error(None)
    with pytest.raises(ValueError):
        B.Regrouper("cuda:0", 4, B.Options(mode="file"))                             # refused before a device is touched
    with pytest.raises(B.BucketError):
        B.Scatter("cpu")


def test_loops_refuse_what_bucketing_excludes():
    from types import SimpleNamespace

    import torch

    from chimeralm_amd import bucket as B, longread as LR, predict as loop

    opt = B.Options()
    dm = SimpleNamespace(tokenizer=SimpleNamespace(padding_side="left"), batch_size_per_device=4)
    right = SimpleNamespace(tokenizer=SimpleNamespace(padding_side="right"), batch_size_per_device=4)
    feeder = SimpleNamespace(pad_left=False, batch_size=4)
    device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="long_reads"):
        loop.run_predict(None, dm, None, device, batching=opt, long_reads=LR.Options(window=64, overlap=0, max_bases=64))
    with pytest.raises(ValueError, match="gathered"):
        loop.run_predict(None, dm, None, device, batching=opt, gather=True)
    with pytest.raises(ValueError, match="left"):
        loop.run_predict(None, right, None, device, batching=opt)
    with pytest.raises(ValueError, match="left"):
        loop.run_predict_native(None, feeder, None, device, batching=opt)
    with pytest.raises(ValueError, match="gathered"):
        loop.run_predict_native(None, SimpleNamespace(pad_left=True, batch_size=4), None, device, batching=opt, on_batch=print)


# ------------------------------------------------------------------------------------------------ the interfaces
def test_header_native_and_exports(built_lib):
    from chimeralm_amd import _native as N, bucket as B, build

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    declared = set(re.findall(r"\b(clm_bucket_[a-z_]+)\s*\(", header))
    assert declared == {"clm_bucket_length", "clm_bucket_pool_bytes", "clm_bucket_plan_create", "clm_bucket_plan_push",
                        "clm_bucket_plan_finish", "clm_bucket_plan_steps", "clm_bucket_plan_last_error", "clm_bucket_plan_destroy",
                        "clm_bucket_create", "clm_bucket_scatter", "clm_bucket_last_error", "clm_bucket_destroy"}
    lib = ctypes.CDLL(str(built_lib))
    for name in declared:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS
    assert {"bucket.hip", "bucket_plan.cpp"} <= set(build.SOURCES)
    assert B.SPAN_DTYPE.itemsize == ctypes.sizeof(N.ClmBucketSpan) == 24 and B.STEP_DTYPE.itemsize == ctypes.sizeof(N.ClmBucketStep) == 32
    assert N.ABI_VERSION == lib.clm_abi_version() and f"#define CLM_ABI_VERSION {N.ABI_VERSION}" in header
    assert "#include <hip" not in (CSRC / "bucket_plan.cpp").read_text() and "clm_common.h" not in (CSRC / "bucket_plan.cpp").read_text()


def test_scatter_kernel_has_no_scratch(built_lib):
    from chimeralm_amd import build

    blocks = [b for b in build.RESOURCES.read_text().split("Function Name: ")[1:] if "bucket" in b.splitlines()[0]]
    assert len(blocks) == 1 and "bucket_scatter_kernel" in blocks[0].splitlines()[0]
    assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[0]).group(1) == "0"
    assert re.search(r"LDS Size \[bytes/block\]: (\d+)", blocks[0]).group(1) == "0"


def test_cli_refusals(tmp_path):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    runner = CliRunner()
    bam = str(tmp_path / "reads.bam")
    for args, text in ((["--batching", "length"], "--batching"),
                       (["--batching", "bucket", "--long-reads", "tile"], "--long-reads"),
                       (["--batching", "bucket", "--gather-logits"], "--gather-logits"),
                       (["--batching", "bucket", "--bucket-steps", "6"], "--bucket-steps")):
        r = runner.invoke(app, ["predict", bam, *args])
        assert r.exit_code == 2, (args, r.output)
        assert text in r.output, (args, r.output)
    r = runner.invoke(app, ["predict", "--help"], env={"COLUMNS": "200", "TERM": "dumb", "NO_COLOR": "1"})
    assert r.exit_code == 0 and "--batching" in r.output and "--bucket-steps" in r.output


def test_eval_py_batching_keys():
    import eval as ev

    with pytest.raises(ValueError, match="steps"):
        ev.batching_options({"batching": {"mode": "bucket", "steps": 3}})
    with pytest.raises(ValueError):
        ev.batching_options({"batching": {"mode": "bucket", "steps_log2": 9}})
    with pytest.raises(ValueError):
        ev.batching_options({"batching": {"mode": "sorted"}})
    assert ev.batching_options({}) is None and ev.batching_options({"batching": {"mode": "file"}}) is None
    opt = ev.batching_options({"batching": {"mode": "bucket", "steps_log2": 2}})
    assert (opt.mode, opt.steps_log2) == ("bucket", 2) and ev.batching_options({"batching": {"mode": "bucket"}}).steps_log2 == 3


def test_sanitizer_program(tmp_path):
    exe = tmp_path / "bucket_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{REPO / 'include'}", str(CSRC / "bucket_plan.cpp"), str(REPO / "tests/sanitize/bucket_host.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "bucket host driver OK" in r.stdout
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert marker not in r.stderr, r.stderr[-4000:]
