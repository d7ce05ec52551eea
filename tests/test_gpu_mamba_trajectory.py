"""The Mamba nets' running verdict on MI355X (csrc/mamba_verdict.hip through clm_mamba_forward_traj) against the literal fp64
reference of tests/mamba_trajectory_reference.py: one whole fp64 forward of the truncated batch per point."""
from __future__ import annotations

import ctypes as C
import functools
import io
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mamba_reference as mr
import mamba_trajectory_reference as MT
import trajectory_reference as TR

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # every point, both precisions: test_gpu_mamba.py's bound on the forward, which each point is on a shorter row
SEED = {"mamba": 31, "mambasp": 32}
# name: (L, S, [PAD]s in front of each row, masked (`mamba` only))  -- the edges of the 64-token tile and of the 128-token point
CASES = {
    "l1": (1, 128, (0, 0), False),
    "l128": (128, 128, (0, 0), False),
    "l129": (129, 128, (0, 0), False),
    "l191": (191, 128, (17, 17), False),
    "l192": (192, 128, (17, 17), False),
    "l193": (193, 128, (17, 17), False),
    "l300s256": (300, 256, (17, 17), False),
    "l777": (777, 128, (0, 300, 777), True),                  # the last row is [PAD] alone; zeros of the mask enter the running maximum
}


def _module(variant, sd, prec, stride=None, **shape):
    from chimeralm_amd import mamba

    d, nl, ds, ex, mml = mr.VARIANTS[variant]
    d, nl, ds = shape.get("d_model") or d, shape.get("n_layers") or nl, shape.get("d_state") or ds
    if variant == "mamba":
        net = mamba.MambaSequenceClassification(vocab_size=12, embedding_dim=d, number_of_layers=nl, model_max_length=mml, dropout=0.1,
                                                number_of_classes=2, d_state=ds, expand=ex, precision=prec, trajectory_stride=stride)
    else:
        net = mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=d, number_of_layers=nl, number_of_classes=2, dropout=0.2,
                                                  d_state=ds, expand=ex, precision=prec, trajectory_stride=stride)
    net.load_state_dict(sd, strict=True)
    return net


@functools.lru_cache(maxsize=None)
def _weights(variant):
    return mr.make_mamba_state_dict(variant, SEED[variant])


@functools.lru_cache(maxsize=None)
def _case(variant, name):
    """ids, mask, S and the fp64 trajectory of a case: computed once, shared by both precisions, never written to."""
    L, S, pads, masked = CASES[name]
    ids = mr.synthetic_ids(SEED[variant] * 100 + L, len(pads), L)
    ids[:, -1] = TR.SEP_ID
    for b, p in enumerate(pads):
        ids[b, :p] = TR.PAD_ID
    mask = None
    if masked and variant == "mamba":
        mask = (np.random.default_rng(L).random(ids.shape) > 0.1).astype(np.float32)
    ref = MT.trajectory_fp64(variant, _weights(variant), ids, S, mask=mask, device="cuda")
    for a in (ids, ref) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    return ids, mask, S, ref


@pytest.fixture(scope="module")
def nets(built_lib):
    """The two reference configs in both precisions, built when first asked for and shared by the tests of this file."""
    made = {}

    def get(variant, prec):
        if (variant, prec) not in made:
            made[variant, prec] = _module(variant, _weights(variant), prec)
        return made[variant, prec]

    yield get
    for net in made.values():
        net.close()


def _forward(net, ids, S, mask=None):
    """(logits, trajectory, summary) as numpy, from one forward with the stride set."""
    net.trajectory_stride = S
    x = torch.tensor(np.asarray(ids)).cuda()
    logits = net(x, None if mask is None else torch.tensor(np.asarray(mask)).cuda()).cpu().numpy()
    t = net.last_trajectory
    assert t is not None and t.stride == S and t.length == x.shape[1]
    return logits, t.logits.cpu().numpy(), t.summary.cpu().numpy()


def _check_against(ref, logits, traj, summary, ids, S, what):
    """Every point within TOL * max(1, max |ref| of that point) of the fp64 reference; the worst error is printed first."""
    K = ref.shape[1]
    assert traj.shape == ref.shape and summary.shape == (len(ids), 12)
    assert np.isfinite(traj).all() and np.isfinite(logits).all(), what
    err = np.abs(traj - ref).max(axis=(0, 2))
    bound = TOL * np.maximum(1.0, np.abs(ref).max(axis=(0, 2)))
    k = int(np.argmax(err / bound))
    print(f"{what}: K = {K}, worst |traj - fp64| = {err.max():.2e} (point {k}: {err[k]:.2e} against {bound[k]:.2e}), max |ref| = {np.abs(ref).max():.3g}")
    assert np.array_equal(traj[:, K - 1], logits), what                       # the forward's own logits, bit for bit
    assert (err <= bound).all(), (what, err.tolist(), bound.tolist())
    TR.check_summary(summary, traj, np.asarray(ids), S)


# ------------------------------------------------------------------------------------------------ parity per point
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_every_point_against_the_fp64_forward_of_the_truncated_row(nets, variant, name, prec):
    ids, mask, S, ref = _case(variant, name)
    net = nets(variant, prec)
    logits, traj, summary = _forward(net, ids, S, mask)
    _check_against(ref, logits, traj, summary, ids, S, f"{variant} {prec} {name}")
    net.trajectory_stride = None                                               # the request changes nothing about the logits
    x = torch.tensor(ids).cuda()
    plain = net(x, None if mask is None else torch.tensor(mask).cuda()).cpu().numpy()
    assert net.last_trajectory is None and np.array_equal(plain, logits)


@pytest.mark.parametrize("variant,d_model", [("mamba", 512), ("mambasp", 256)])
def test_other_channel_widths(built_lib, variant, d_model):
    """One layer at the channel width of the other net: both widths in both kernels."""
    sd = mr.make_mamba_state_dict(variant, 33, n_layers=1, d_model=d_model)
    ids = mr.synthetic_ids(3300, 2, 193, pads=17)
    ids[:, -1] = TR.SEP_ID
    ref = MT.trajectory_fp64(variant, sd, ids, 128, device="cuda")
    for prec in ("fp32", "fp16x3"):
        net = _module(variant, sd, prec, n_layers=1, d_model=d_model)
        logits, traj, summary = _forward(net, ids, 128)
        _check_against(ref, logits, traj, summary, ids, 128, f"{variant} d_model {d_model} {prec}")
        net.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("variant,n_layers", [("mamba", 2), ("mambasp", 1)])
def test_interior_points_are_the_forward_of_the_cut_row_bit_for_bit(built_lib, variant, n_layers, prec):
    """The forward's head and the verdict's head run one dense routine (csrc/mamba_common.h head_dense), and everything in front
    of the pooling is causal per 64-token tile: interior point k IS the logits of a forward of the rows cut at (k + 1) * stride."""
    sd = mr.make_mamba_state_dict(variant, 35, d_state=16, n_layers=n_layers)
    ids = mr.synthetic_ids(3500, 2, 384, pads=17)
    net = _module(variant, sd, prec, n_layers=n_layers, d_state=16)
    logits, traj, _ = _forward(net, ids, 128)
    assert traj.shape == (2, 3, 2) and np.isfinite(traj).all() and np.array_equal(traj[:, 2], logits)
    net.trajectory_stride = None
    for k in range(2):
        cut = net(torch.tensor(ids[:, :(k + 1) * 128]).cuda()).cpu().numpy()
        print(f"{variant} {prec} point {k}: max |traj - forward of the cut row| = {np.abs(traj[:, k] - cut).max():.2e}")
        assert np.array_equal(traj[:, k], cut), (variant, prec, k)
    assert np.abs(traj[:, 0] - traj[:, 1]).max() > 1e-6                        # (the points differ)
    net.close()


# ------------------------------------------------------------------------------------------------ chunks, determinism, placement
def test_chunk_offsets(nets):
    """40 x 8,193 on `mambasp` is two chunks of reads (a chunk's in_proj output is bounded at 4 GiB, about 299k tokens here): the
    trajectory and summary of rows 0 and 39 equal those of the same reads run alone, bit for bit."""
    net = nets("mambasp", "fp16x3")
    ids = mr.synthetic_ids(3400, 40, 8193)
    ids[:, -1] = TR.SEP_ID
    for b in range(40):
        ids[b, :(b * 211) % 8000] = TR.PAD_ID
    logits, traj, summary = _forward(net, ids, 4096)
    assert traj.shape == (40, 3, 2) and np.isfinite(traj).all()
    assert np.array_equal(traj[:, 2], logits)
    assert np.abs(traj[:, 0] - traj[:, 1]).max() > 1e-3                        # (the points differ)
    TR.check_summary(summary, traj, ids, 4096)
    for r in (0, 39):
        l1, t1, s1 = _forward(net, ids[r:r + 1], 4096)
        assert np.array_equal(l1[0], logits[r]) and np.array_equal(t1[0], traj[r]) and np.array_equal(s1[0], summary[r]), r


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_two_runs_are_bitwise_equal(nets, variant):
    ids, mask, S, _ = _case(variant, "l777")
    net = nets(variant, "fp16x3")
    a = _forward(net, ids, S, mask)
    b = _forward(net, ids, S, mask)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _raw(net, ids, S, *, point_stride=None, struct_size=None, logits=True, fill=None):
    """clm_mamba_forward_traj on the module's handle: (rc, message, logits, traj [B, point_stride, 2], summary)."""
    from chimeralm_amd import _native as N

    x = torch.tensor(np.asarray(ids)).cuda()
    lib = net._prepare(x.device)
    B, L = x.shape
    K = -(-L // S) if S > 0 else 1
    ps = K if point_stride is None else point_stride
    out = torch.empty((B, 2), dtype=torch.float32, device="cuda")
    traj = torch.full((B, max(ps, 1), 2), np.nan if fill is None else fill, dtype=torch.float32, device="cuda")
    summary = torch.zeros((B, 12), dtype=torch.int32, device="cuda")
    c = N.ClmTrajOut()
    c.struct_size = C.sizeof(N.ClmTrajOut) if struct_size is None else struct_size
    c.stride, c.point_stride, c.summary = S, ps, summary.data_ptr()
    c.logits = traj.data_ptr() if logits else None
    rc = lib.clm_mamba_forward_traj(net._h, C.c_void_p(x.data_ptr()), N.DT_I64, x.stride(0), B, L, None, 0, C.c_void_p(out.data_ptr()),
                                    C.byref(c), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.clm_mamba_last_error(net._h).decode(), out.cpu().numpy(), traj.cpu().numpy(), summary.cpu().numpy()


def test_a_wider_point_stride_leaves_the_gap_untouched(nets):
    ids, _, S, _ = _case("mambasp", "l777")
    net = nets("mambasp", "fp32")
    logits, traj, summary = _forward(net, ids, S)
    K = traj.shape[1]
    rc, msg, l2, wide, s2 = _raw(net, ids, S, point_stride=K + 3, fill=-777.0)
    assert rc == 0, msg
    assert np.array_equal(wide[:, :K], traj) and np.array_equal(l2, logits) and np.array_equal(s2, summary)
    assert (wide[:, K:] == -777.0).all()


def test_errors_through_the_abi(nets):
    from chimeralm_amd import _native as N

    ids, _, _, _ = _case("mambasp", "l300s256")
    net = nets("mambasp", "fp32")
    for kw, S, said in ((dict(), 0, "multiple of 128"), (dict(), 64, "multiple of 128"), (dict(), 192, "multiple of 128"),
                        (dict(), 8192, "multiple of 128"), (dict(point_stride=2), 128, "point_stride"),
                        (dict(logits=False), 128, "no logits buffer"), (dict(struct_size=24), 128, "size mismatch")):
        rc, msg, *_ = _raw(net, ids, S, **kw)
        assert rc == N.E_INVALID and said in msg and msg.startswith("clm_mamba_forward_traj"), (kw, S, rc, msg)
    rc, msg, *_ = _raw(net, ids, 128, point_stride=3)                          # K = 3 fits exactly
    assert rc == 0, msg


# ------------------------------------------------------------------------------------------------ the non-finite rerun
def test_nonfinite_rerun_keeps_the_trajectory_of_the_handle_that_answered(built_lib, caplog):
    """test_gpu_mamba.py's embedding scaled by 2^17: fp16x3 returns NaN, the batch is rerun on the exact-fp32 handle with the
    request made again; the trajectory left is that handle's."""
    ids = mr.synthetic_ids(2500, 2, 300)
    sd = mr.make_mamba_state_dict("mambasp", 26, n_layers=2)
    sd["embedding.weight"] = sd["embedding.weight"] * 131072.0
    net = _module("mambasp", sd, "fp16x3", stride=128, n_layers=2)
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    assert net.precision_report["nonfinite_reruns"] == 1
    t = net.last_trajectory
    traj = t.logits.cpu().numpy()
    assert traj.shape == (2, 3, 2) and np.isfinite(got).all() and np.isfinite(traj).all()
    assert np.array_equal(traj[:, -1], got)
    TR.check_summary(t.summary.cpu().numpy(), traj, ids, 128)
    exact = _module("mambasp", sd, "fp32", stride=128, n_layers=2)
    assert np.array_equal(exact(torch.from_numpy(ids).cuda()).cpu().numpy(), got)
    assert np.array_equal(exact.last_trajectory.logits.cpu().numpy(), traj)
    net.close()
    exact.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_eval_py_route(tmp_path, golden_dir, built_lib):
    """`eval.py ... model=mambasp +trajectory.stride=128 +trajectory.values=true` writes, next to unchanged predictions, the files
    `TrajectoryWriter` writes for the same batches through the Python API."""
    from chimeralm_amd import bam, tokenizer as T
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.callbacks import TrajectoryWriter

    repo = Path(__file__).resolve().parent.parent
    sd = {f"net.{k}": v for k, v in mr.make_mamba_state_dict("mambasp", 28).items()}
    ckpt = tmp_path / "mambasp.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    env = {**os.environ, "PYTHONPATH": str(repo)}
    base = [sys.executable, str(repo / "eval.py"), f"ckpt_path={ckpt}", "model=mambasp",
            f"+data.predict_data_path={golden_dir / 'test_chimric_reads.bam'}", "data.batch_size=10", "+data.max_predict_samples=20",
            "model.net.precision=fp32"]
    for out, extra in ((tmp_path / "plain", []), (tmp_path / "run", ["+trajectory.stride=128", "+trajectory.values=true"])):
        r = subprocess.run(base + [f"hydra.run.dir={out}"] + extra, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    plain, run = tmp_path / "plain" / "predicts", tmp_path / "run" / "predicts"
    assert sorted(p.name for p in plain.iterdir()) == ["0_0.txt", "0_1.txt"]
    assert sorted(p.name for p in run.iterdir()) == ["0_0.traj.npz", "0_0.traj.tsv", "0_0.txt", "0_1.traj.npz", "0_1.traj.tsv", "0_1.txt"]
    for name in ("0_0.txt", "0_1.txt"):
        assert (run / name).read_bytes() == (plain / name).read_bytes()
    net = _module("mambasp", mr.make_mamba_state_dict("mambasp", 0), "fp32", stride=128)
    model = ClassificationLit(net).load_reference_checkpoint(ckpt)
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / "test_chimric_reads.bam", batch_size=10, max_predict_samples=20)
    dm.setup("predict")
    api = TrajectoryWriter(tmp_path / "api", values=True)
    for i, batch in enumerate(dm.predict_dataloader()):
        model.predict_step({**batch, "input_ids": batch["input_ids"].cuda()}, i)
        host = net.last_trajectory.to_host()
        torch.cuda.synchronize()
        api.write_on_batch_end(SimpleNamespace(global_rank=0), host, batch, i)
        assert (run / f"0_{i}.traj.tsv").read_bytes() == (tmp_path / "api" / f"0_{i}.traj.tsv").read_bytes()
        got = np.load(io.BytesIO((run / f"0_{i}.traj.npz").read_bytes()))
        want = np.load(io.BytesIO((tmp_path / "api" / f"0_{i}.traj.npz").read_bytes()))
        assert sorted(got.files) == sorted(want.files) == ["bases_seen", "names", "traj"]
        for key in want.files:
            assert np.array_equal(got[key], want[key]), key
        assert got["traj"].shape[0] == 10 and got["traj"].shape[1] == -(-batch["input_ids"].shape[1] // 128)
    net.close()
