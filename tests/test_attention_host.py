"""CPU: attention as an output -- the binding of the new entry points, the numpy reference of the summary and peaks
(tests/attn_reference.py), the bytes `AttentionWriter` writes, `filter` next to those files, and the command line."""
from __future__ import annotations

import ctypes
import io
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import torch

from attn_reference import softmax64, summarize

REPO = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------- binding
def test_attention_entry_points_are_exported_declared_and_bound(built_lib, tmp_path):
    from chimeralm_amd import _native as N

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    lib = ctypes.CDLL(str(built_lib))
    for name in ("clm_forward_attn", "clm_forward_staged_attn"):
        assert hasattr(lib, name), f"{name} not exported"
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} not declared"
        assert name in N.SYMBOLS
    assert "typedef struct clm_attn_out" in header and "typedef struct clm_attn_summary" in header
    assert N.load().clm_abi_version() == 6 == N.ABI_VERSION and "#define CLM_ABI_VERSION 6" in header
    # the ctypes mirrors have the layout the C compiler gives the header's structs
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chimeralm_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(clm_attn_summary), sizeof(clm_attn_out), offsetof(clm_attn_out, weights), "
                   "offsetof(clm_attn_out, summary), offsetof(clm_attn_out, peak_weight)); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", f"-I{REPO / 'include'}", str(src), "-o", str(tmp_path / "sizes")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sizes")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(N.ClmAttnSummary), ctypes.sizeof(N.ClmAttnOut), N.ClmAttnOut.weights.offset,
                   N.ClmAttnOut.summary.offset, N.ClmAttnOut.peak_weight.offset] and got[0] == 32


def test_attention_request_arguments():
    import pytest

    from chimeralm_amd.engine import AttentionRequest

    assert AttentionRequest().top_k == 10 and not AttentionRequest().weights
    for bad in (dict(top_k=0), dict(top_k=33), dict(top_k=None, weights=False)):
        with pytest.raises(ValueError):
            AttentionRequest(**bad)


# ---------------------------------------------------------------------------------------------- the numpy reference
def test_peak_reference_is_argsort_on_the_bases():
    rng = np.random.default_rng(3)
    for L, n_pad, top_k in ((50, 0, 10), (300, 17, 10), (40, 30, 32), (12, 0, 5), (9, 6, 10)):
        w = softmax64(rng.normal(0, 3, L)).astype(np.float32)
        ids = rng.integers(7, 11, L)
        ids[:n_pad], ids[-1] = 4, 1
        r = summarize(w, ids, top_k)
        bases = w[n_pad:-1]
        assert len(set(bases.tolist())) == len(bases)                            # (no ties: argsort is unambiguous)
        assert r["pos"] == np.argsort(bases)[-top_k:][::-1].tolist()             # notebooks/attention.ipynb find_attention_peaks
        assert (r["n_pad"], r["n_bases"], r["has_sep"], r["n_peaks"]) == (n_pad, L - n_pad - 1, 1, min(top_k, L - n_pad - 1))
        assert abs(r["pad_weight"] + r["sep_weight"] + r["base_weight"] - 1.0) < 1e-6
        assert abs(r["sep_weight"] - float(w[-1])) == 0


def test_peak_reference_tie_rule_and_edges():
    w = np.array([0.05, 0.2, 0.1, 0.2, 0.1, 0.2, 0.05, 0.1], np.float32)
    ids = np.array([4, 8, 8, 9, 7, 10, 7, 1])
    r = summarize(w, ids, 4)
    assert r["pos"] == [0, 2, 4, 1] and [float(x) for x in r["weight"]] == [float(np.float32(x)) for x in (0.2, 0.2, 0.2, 0.1)]
    assert (r["n_pad"], r["n_bases"], r["has_sep"]) == (1, 6, 1)
    assert summarize(w, ids, 32)["pos"] == [0, 2, 4, 1, 3, 5]                    # top_k > n_bases: every base, once
    allpad = summarize(np.full(4, 0.25, np.float32), np.array([4, 4, 4, 4]), 10)
    assert (allpad["n_pad"], allpad["n_bases"], allpad["has_sep"], allpad["n_peaks"], allpad["pos"]) == (4, 0, 0, 0, [])
    only_sep = summarize(np.ones(1, np.float32), np.array([1]), 10)
    assert (only_sep["n_pad"], only_sep["n_bases"], only_sep["has_sep"], only_sep["sep_weight"]) == (0, 0, 1, 1.0)
    no_sep = summarize(np.array([0.5, 0.5], np.float32), np.array([7, 8]), 10)   # a 4 inside the read is a base, not a pad
    assert (no_sep["n_bases"], no_sep["has_sep"], no_sep["pos"]) == (2, 0, [0, 1])
    inner = summarize(np.array([0.1, 0.2, 0.3, 0.4], np.float32), np.array([4, 7, 4, 1]), 10)
    assert (inner["n_pad"], inner["n_bases"], inner["pos"]) == (1, 2, [1, 0])
    nan = summarize(np.array([0.5, np.nan, 0.5], np.float32), np.array([7, 7, 1]), 10)
    assert nan["n_peaks"] == 0 and nan["pos"] == [] and np.isnan(nan["base_weight"])


def test_peak_reference_on_the_reference_heads_weights(golden_dir):
    """tests/golden/head_golden.npz `attn_*`: `attention_weights` of the reference's BinarySequenceClassifier (save_attention)."""
    z = np.load(golden_dir / "head_golden.npz")
    for key in ("attn_0", "attn_1"):
        for row in z[key][..., 0]:
            ids = np.full(len(row), 8)
            ids[-1] = 1
            r = summarize(row, ids, 10)
            assert r["pos"] == np.argsort(row[:-1])[-10:][::-1].tolist()
            assert abs(r["base_weight"] + r["sep_weight"] - 1.0) < 1e-5 and r["pad_weight"] == 0.0
            assert all(a >= b for a, b in zip(r["weight"], r["weight"][1:]))


# ---------------------------------------------------------------------------------------------- the writer
def _name_row(name: bytes, width: int) -> list[int]:
    return [len(name)] + list(name) + [0] * (width - 1 - len(name))


def _host_attention(rows, top_k, weights=None):
    from chimeralm_amd.engine import AttentionOutput

    summary = torch.zeros((len(rows), 8), dtype=torch.int32)
    pos = torch.full((len(rows), top_k), -1, dtype=torch.int32)
    pw = torch.zeros((len(rows), top_k), dtype=torch.float32)
    for i, r in enumerate(rows):
        summary[i, :4] = torch.tensor([r["n_pad"], r["n_bases"], r["has_sep"], len(r["peaks"])], dtype=torch.int32)
        summary.view(torch.float32)[i, 4:7] = torch.tensor([r["pad_w"], r["sep_w"], r["base_w"]])
        for k, (p, w) in enumerate(r["peaks"]):
            pos[i, k], pw[i, k] = p, w
    return AttentionOutput(top_k, summary, pos, pw, None if weights is None else torch.from_numpy(weights))


def test_attention_writer_bytes(tmp_path):
    from types import SimpleNamespace

    from chimeralm_amd.callbacks import AttentionWriter

    long_name = b"r" * 130 + b"/1"                                              # > 127 characters: the length byte is unsigned
    width = 140
    ids = torch.tensor([_name_row(long_name, width), [0] * width, _name_row(b"\x01\x02", width), _name_row(b"read_d", width)],
                       dtype=torch.uint8)
    third = float(np.float32(1.0) / np.float32(3.0))
    rows = [
        dict(n_pad=2, n_bases=5, has_sep=1, pad_w=0.125, sep_w=0.0625, base_w=0.8125, peaks=[(3, 0.5), (0, 0.25), (4, third)]),
        dict(n_pad=0, n_bases=2, has_sep=1, pad_w=0.0, sep_w=0.5, base_w=0.5, peaks=[(0, 0.25), (1, 0.25)]),   # top_k > n_bases
        dict(n_pad=7, n_bases=0, has_sep=1, pad_w=0.75, sep_w=0.25, base_w=0.0, peaks=[]),                      # no bases
        dict(n_pad=0, n_bases=3, has_sep=0, pad_w=0.0, sep_w=0.0, base_w=1.0, peaks=[(2, 1e-7), (0, 0.0), (1, 0.0)]),
    ]
    L = 8
    w = np.zeros((4, L), np.float32)
    w[0, 2:7] = [0.25, 0.01, 0.02, 0.5, third]
    w[1, 0:2] = [0.25, 0.25]
    w[3, 0:3] = [0.0, 0.0, 1e-7]
    logits = torch.tensor([[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [-1.0, 2.0]])
    batch = {"id": ids, "labels": torch.full((4,), -1)}
    want = (f"{long_name.decode()}\t1\t5\t2\t0.125\t0.0625\t3:0.5;0:0.25;4:0.333333\n"
            "error_read_1\t0\t2\t0\t0\t0.5\t0:0.25;1:0.25\n"
            "unknown_read_2\t0\t0\t7\t0.75\t0.25\t\n"
            "read_d\t1\t3\t0\t0\t0\t2:1e-07;0:0;1:0\n")
    out = tmp_path / "pred"
    AttentionWriter(out).write_on_batch_end(SimpleNamespace(global_rank=3), None, (logits, batch["labels"]),
                                            _host_attention(rows, 4), batch, 7)
    assert (out / "3_7.attn.tsv").read_bytes() == want.encode()
    assert sorted(p.name for p in out.iterdir()) == ["3_7.attn.tsv"]             # no npz unless asked for, nothing named *.txt
    wr = AttentionWriter(out, weights=True)
    wr.write_on_batch_end(None, None, (logits, batch["labels"]), _host_attention(rows, 4, w), batch, 0)
    assert (out / "0_0.attn.tsv").read_bytes() == want.encode()
    raw = (out / "0_0.attn.npz").read_bytes()
    z = np.load(io.BytesIO(raw))
    assert sorted(z.files) == ["n_bases", "names", "offsets", "weights"]
    assert z["names"].tolist() == [long_name.decode(), "error_read_1", "unknown_read_2", "read_d"]
    assert z["n_bases"].dtype == np.int32 and z["n_bases"].tolist() == [5, 2, 0, 3]
    assert z["offsets"].dtype == np.int64 and z["offsets"].tolist() == [0, 5, 7, 7, 10]
    assert z["weights"].dtype == np.float32
    assert z["weights"].tobytes() == np.concatenate([w[0, 2:7], w[1, 0:2], w[3, 0:3]]).tobytes()   # pads and [SEP] stripped
    wr.write_on_batch_end(None, None, (logits, batch["labels"]), _host_attention(rows, 4, w), batch, 0)
    assert (out / "0_0.attn.npz").read_bytes() == raw                            # the same bytes every time (no time stamps)


# ---------------------------------------------------------------------------------------------- filter, command line
def test_filter_does_not_see_attention_files(tmp_path, golden_dir, built_lib):
    from chimeralm_amd import filter as flt

    def run(with_attention: bool):
        d = tmp_path / ("with" if with_attention else "without")
        d.mkdir()
        bam = d / "reads.bam"
        shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
        pred = d / "reads.predictions"
        pred.mkdir()
        names = _bam_names(bam)
        (pred / "0_0.txt").write_text("".join(f"{n}\t{(i % 3 == 0) * 1}\n" for i, n in enumerate(names)))
        if with_attention:                                                       # labels that would flip every read if they were read
            (pred / "0_0.attn.tsv").write_text("".join(f"{n}\t{(i % 3 != 0) * 1}\t5\t0\t0\t0.5\t0:0.5\n" for i, n in enumerate(names)))
            np.savez(pred / "0_0.attn.npz", names=np.asarray(names), weights=np.zeros(3, np.float32))
        res = flt.filter_bam_by_predcition(bam, pred, index=True, output_prediction=True)
        return (res["kept"], res["dropped"], res["filtered"].read_bytes(), res["sorted"].read_bytes(),
                Path(str(res["sorted"]) + ".bai").read_bytes(), (pred / "predictions.txt").read_bytes())

    a, b = run(False), run(True)
    assert a == b and a[1] > 0


def _bam_names(bam: Path) -> list[str]:
    """Read names of a BAM in file order, each once (SAM specification 4.2; BGZF members are gzip members)."""
    import gzip
    import struct

    data = gzip.decompress(bam.read_bytes())
    assert data[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", data, p)[0]
    names = []
    while p < len(data):
        size = struct.unpack_from("<i", data, p)[0]
        l_name = data[p + 12]
        names.append(data[p + 36: p + 36 + l_name - 1].decode())
        p += 4 + size
    return list(dict.fromkeys(names))


def test_predict_help_lists_the_attention_options():
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    r = CliRunner().invoke(app, ["predict", "--help"], env={"COLUMNS": "200", "NO_COLOR": "1", "TERM": "dumb"})
    assert r.exit_code == 0
    text = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    for opt in ("--save-attention", "--attention-top-k", "--attention-weights"):
        assert opt in text, opt
    assert re.search(r"--attention-top-k.*\b10\b", text.replace("\n", " "))       # the notebook's default
