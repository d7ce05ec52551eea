"""CPU: the running verdict's references, ABI, writer and refusals (csrc/trajectory.hip; the GPU side: test_gpu_trajectory.py)."""
from __future__ import annotations

import ctypes
import io
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import trajectory_reference as TR
from oracle import hyena_oracle as ho

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("L", [40, 130, 300])
def test_prefix_pooling_on_the_oracle_is_the_forward_of_the_prefix(L):
    """head(backbone(ids)[:, :n_k]) = forward(ids[:, :n_k]) to 1e-9 in fp64: the oracle's backbone is causal, so pooling a prefix of
    the final residual stream is what the model would compute on the truncated row."""
    sd = ho.make_state_dict(0, head_scale=3.0)
    ids = TR.padded_batch(L, (0, L // 3), seed=L)
    ref = TR.trajectory_fp64(ids, sd, 128)
    n_k = TR.points(L, 128)
    assert ref.shape == (2, len(n_k), 2) and n_k[-1] == L
    for k, n in enumerate(n_k):
        literal = ho.forward(torch.from_numpy(ids[:, :n].astype(np.int64)), sd, torch.float64).numpy()
        assert np.abs(ref[:, k] - literal).max() <= 1e-9, (L, k)
    assert len(n_k) == 1 or np.abs(np.diff(ref[:, :, 1] - ref[:, :, 0], axis=1)).max() > 1e-3   # (the curve moves: the test says something)


def test_points():
    assert TR.points(1, 128) == [1] and TR.points(128, 128) == [128] and TR.points(129, 128) == [128, 129]
    assert TR.points(300, 256) == [256, 300] and len(TR.points(8193, 128)) == 65 and len(TR.points(32769, 128)) == 257
    assert TR.bases_seen(3, 128, 300, 130, 169) == [0, 126, 169] and TR.bases_seen(1, 128, 1, 1, 0) == [0]


# ------------------------------------------------------------------------------------------------ the summary reference
def _curve(gaps):
    g = np.asarray(gaps, np.float32)
    return np.stack([np.zeros_like(g), g], axis=1)


def _ids(L, n_pad, sep=True):
    ids = np.full(L, 8, np.uint8)
    ids[:n_pad] = 4
    if sep:
        ids[-1] = 1
    return ids


def test_summary_on_hand_made_curves():
    S = 128
    # a verdict that flips twice: 5 points, label 1, the run of the final label starts at point 3; the largest step up is 1 -> 2? no:
    # steps are +3 (into 1), -4 (into 2), +2.5 (into 3), +0.5 (into 4): jump at point 1
    r = TR.summarize(_curve([-1, 2, -2, 0.5, 1]), _ids(600, 0), S)
    assert (r["n_points"], r["first_k"], r["label"], r["onset_k"], r["jump_k"]) == (5, 0, 1, 3, 1)
    assert r["jump_dgap"] == np.float32(3) and r["final_gap"] == np.float32(1) and r["n_nonfinite"] == 0
    assert (r["n_pad"], r["n_bases"], r["has_sep"]) == (0, 599, 1)
    # label 0: the sign turns the steps round; ties go to the lowest k (two steps of -2)
    r = TR.summarize(_curve([1, -1, 0.5, -1.5, -1.5]), _ids(600, 0, sep=False), S)
    assert (r["label"], r["onset_k"], r["jump_k"], r["has_sep"], r["n_bases"]) == (0, 3, 1, 0, 600) and r["jump_dgap"] == np.float32(2)
    # a tie in the final gap is class 0, and a point with gap 0 carries label 0
    r = TR.summarize(_curve([0, 1, 0, 0]), _ids(512, 0), S)
    assert (r["label"], r["onset_k"], r["jump_k"]) == (0, 2, 2) and r["jump_dgap"] == np.float32(1) and r["final_gap"] == 0
    # points inside the [PAD] prefix do not count: 300 pads of 640 tokens -> first_k = 2; the early flip at point 1 is not seen
    r = TR.summarize(_curve([5, -5, 1, 2, 3]), _ids(640, 300), S)
    assert (r["n_pad"], r["first_k"], r["onset_k"], r["jump_k"]) == (300, 2, 2, 3) and r["jump_dgap"] == np.float32(1)
    # a single informative point: nothing to step from
    r = TR.summarize(_curve([5, -5, 1]), _ids(384, 256), S)
    assert (r["first_k"], r["onset_k"], r["jump_k"]) == (2, 2, -1) and r["jump_dgap"] == 0
    r = TR.summarize(_curve([2]), _ids(100, 0), S)
    assert (r["n_points"], r["first_k"], r["onset_k"], r["jump_k"], r["label"]) == (1, 0, 0, -1, 1)
    # an all-[PAD] row: first_k is the last point
    r = TR.summarize(_curve([1, 2, 3]), _ids(300, 300, sep=False), S)
    assert (r["n_pad"], r["n_bases"], r["first_k"], r["jump_k"]) == (300, 0, 2, -1)
    # NaN behind the prefix: counted, no onset, no jump; NaN inside the prefix: not counted
    r = TR.summarize(_curve([1, np.nan, 3, np.inf]), _ids(512, 0), S)
    assert (r["n_nonfinite"], r["onset_k"], r["jump_k"]) == (2, -1, -1) and r["jump_dgap"] == 0
    r = TR.summarize(_curve([np.nan, 1, 3, 4]), _ids(512, 128), S)
    assert (r["n_nonfinite"], r["first_k"], r["onset_k"], r["jump_k"]) == (0, 1, 1, 2)
    r = TR.summarize(_curve([1, 2, np.nan]), _ids(384, 0), S)
    assert r["label"] == 0 and r["n_nonfinite"] == 1 and np.isnan(r["final_gap"])
    # a stride of 256
    r = TR.summarize(_curve([-1, 1]), _ids(300, 130), 256)
    assert (r["n_points"], r["first_k"], r["onset_k"], r["jump_k"]) == (2, 0, 1, 1) and r["jump_dgap"] == np.float32(2)


def test_check_summary_compares_every_field():
    ids = np.stack([_ids(384, 0), _ids(384, 200)])
    traj = np.stack([_curve([-1, 2, 1]), _curve([3, -1, -2])])
    rec = np.zeros((2, 12), np.int32)
    for b in range(2):
        r = TR.summarize(traj[b], ids[b], 128)
        rec[b, :10] = [r[n] for n in TR.FIELDS[:10]]
        rec[b, 10:] = np.array([r["jump_dgap"], r["final_gap"]], np.float32).view(np.int32)
    TR.check_summary(rec, traj, ids, 128)
    rec[1, 6] += 1
    with pytest.raises(AssertionError):
        TR.check_summary(rec, traj, ids, 128)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_native_and_exports(built_lib):
    from chimeralm_amd import _native as N, build, engine as E

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    lib = ctypes.CDLL(str(built_lib))
    for name in ("clm_forward_traj", "clm_forward_staged_traj"):
        assert hasattr(lib, name) and name in N.SYMBOLS and f"int {name}(" in header
    assert "#define CLM_ABI_VERSION 6" in header and N.ABI_VERSION == 6 and lib.clm_abi_version() == 6   # new symbols only
    assert "trajectory.hip" in build.SOURCES and "head_dense.h" in build.HEADERS
    assert ctypes.sizeof(N.ClmTrajSummary) == 48 == 4 * len(E.TRAJ_FIELDS) and ctypes.sizeof(N.ClmTrajOut) == 32
    assert [n for n, _ in N.ClmTrajSummary._fields_] == list(E.TRAJ_FIELDS) == list(TR.FIELDS)
    for text in ("does not end in [SEP]", "describe pads only", "precision, fall-back level, short-read switch"):
        assert text in header
    blocks = [b for b in build.RESOURCES.read_text().split("Function Name: ")[1:] if "traj_" in b.splitlines()[0]]
    assert len(blocks) == 3                                     # prefix merge, classifier, summary
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1) == "0", b.splitlines()[0]


def test_requests():
    from chimeralm_amd import lm
    from chimeralm_amd.engine import TrajectoryRequest, bases_seen

    for bad in (0, 64, 127, 192, 4224, 8192):
        with pytest.raises(ValueError, match="multiple of 128"):
            TrajectoryRequest(stride=bad)
        with pytest.raises(ValueError, match="multiple of 128"):
            lm.ChimeraLM.new(trajectory_stride=bad)
    assert TrajectoryRequest().stride == 128 and TrajectoryRequest(4096).summary
    net = lm.ChimeraLM.new(trajectory_stride=256).net
    assert net.trajectory_request() == TrajectoryRequest(256, True) and net.last_trajectory is None
    assert lm.ChimeraLM.new().net.trajectory_request() is None
    assert bases_seen(3, 128, 300, [130, 0], [169, 299]).tolist() == [TR.bases_seen(3, 128, 300, 130, 169), TR.bases_seen(3, 128, 300, 0, 299)]


# ------------------------------------------------------------------------------------------------ the writer
def _pack_names(names):
    from chimeralm_amd.tokenizer import pack_read_name

    return torch.from_numpy((np.asarray([pack_read_name(n) for n in names], dtype=np.int64) & 0xFF).astype(np.uint8).view(np.int8))


def test_trajectory_writer_bytes(tmp_path):
    from chimeralm_amd.callbacks import TrajectoryWriter
    from chimeralm_amd.engine import TrajectoryOutput

    L, S = 600, 128
    ids = np.stack([_ids(L, 0), _ids(L, 300), _ids(L, 599)])
    traj = np.stack([_curve([-1, 2, -2, 0.5, 1]), _curve([5, -5, -1.25, -2, np.nan]), _curve([0, 0, 0, 0, -0.5])]).astype(np.float32)
    rec = np.zeros((3, 12), np.int32)
    for b in range(3):
        r = TR.summarize(traj[b], ids[b], S)
        rec[b, :10] = [r[n] for n in TR.FIELDS[:10]]
        rec[b, 10:] = np.array([r["jump_dgap"], r["final_gap"]], np.float32).view(np.int32)
    out = TrajectoryOutput(S, L, torch.from_numpy(traj), torch.from_numpy(rec))
    batch = {"id": _pack_names(["read/0", "b", "sep-only"])}
    TrajectoryWriter(tmp_path, values=True).write_on_batch_end(SimpleNamespace(global_rank=1), out, batch, 4)
    want = ("read/0\t1\t599\t5\t128\t512\t128\t256\t3\t1\n"          # settles at point 3 (512 bases seen), steps most into point 1
            "b\t0\t299\t5\t84\t-1\t-1\t-1\t0\tnan\n"                  # a NaN behind the prefix: no onset, no jump
            "sep-only\t0\t0\t5\t0\t0\t-1\t-1\t0\t-0.5\n")             # one informative point, which holds [SEP] alone
    assert (tmp_path / "1_4.traj.tsv").read_bytes() == want.encode()
    z = np.load(io.BytesIO((tmp_path / "1_4.traj.npz").read_bytes()))
    assert z["names"].tolist() == ["read/0", "b", "sep-only"] and z["traj"].dtype == np.float32 and z["bases_seen"].dtype == np.int32
    assert np.array_equal(z["traj"], traj, equal_nan=True)
    assert z["bases_seen"].tolist() == [[128, 256, 384, 512, 599], [0, 0, 84, 212, 299], [0, 0, 0, 0, 0]]
    assert not list(tmp_path.glob("*.txt"))                     # `filter` globs *.txt
    TrajectoryWriter(tmp_path / "plain").write_on_batch_end(None, out, batch, 0)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["0_0.traj.tsv"]
    assert (tmp_path / "plain" / "0_0.traj.tsv").read_bytes() == want.encode()


# ------------------------------------------------------------------------------------------------ refusals
def test_cli_refusals(tmp_path):
    from typer.testing import CliRunner

    from chimeralm_amd.__main__ import app

    runner = CliRunner()
    bam = str(tmp_path / "reads.bam")
    for args, text in ((["--save-trajectory", "--long-reads", "tile"], "--save-trajectory"),
                       (["--trajectory-values", "--long-reads", "tile"], "--save-trajectory"),
                       (["--save-trajectory", "--trajectory-stride", "192"], "--trajectory-stride"),
                       (["--save-trajectory", "--trajectory-stride", "8192"], "--trajectory-stride")):
        r = runner.invoke(app, ["predict", bam, *args])
        assert r.exit_code == 2, (args, r.output)
        assert text in r.output, (args, r.output)
    r = runner.invoke(app, ["predict", "--help"], env={"COLUMNS": "200", "TERM": "dumb", "NO_COLOR": "1"})
    assert r.exit_code == 0 and all(o in r.output for o in ("--save-trajectory", "--trajectory-stride", "--trajectory-values"))


def test_loops_refuse_nets_that_are_not_causal_and_tiled_reads(tmp_path):
    from chimeralm_amd import cnn, lm, longread, predict
    from chimeralm_amd.callbacks import PredictionWriter, TrajectoryWriter

    tw, dev = TrajectoryWriter(tmp_path), torch.device("cpu")
    conv = cnn.DNAConvNet(**cnn.PRODUCTION)
    with pytest.raises(ValueError, match="causal"):
        predict.run_predict(SimpleNamespace(net=conv), None, PredictionWriter(tmp_path), dev, trajectory_writer=tw)
    with pytest.raises(ValueError, match="causal"):
        predict.run_predict_native(SimpleNamespace(net=conv), None, PredictionWriter(tmp_path), dev, trajectory_writer=tw)
    model = lm.ChimeraLM.new(trajectory_stride=128)
    tile = longread.Options(mode="tile", window=1024, overlap=128, max_bases=4096)
    with pytest.raises(ValueError, match="single row"):
        predict.run_predict(model, None, PredictionWriter(tmp_path), dev, trajectory_writer=tw, long_reads=tile)
    with pytest.raises(ValueError, match="single row"):
        predict.run_predict_native(model, None, PredictionWriter(tmp_path), dev, trajectory_writer=tw, long_reads=tile)
    with pytest.raises(ValueError, match="trajectory_stride"):
        predict.run_predict(lm.ChimeraLM.new(), None, PredictionWriter(tmp_path), dev, trajectory_writer=tw)
    assert predict._trajectory_setup(model, None) is None and predict._trajectory_setup(model, tw).stride == 128
