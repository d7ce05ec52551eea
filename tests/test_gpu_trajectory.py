"""GPU (MI355X): the running verdict -- prefix logits along a read from one forward (csrc/trajectory.hip, clm_forward_traj; DESIGN.md
section 5.10).

Bounds.  fp32 and fp16x3: every interior point within 1e-4 of the fp64 reference (the oracle's head on the first n_k rows of the
oracle's residual stream), the project's bound for these arithmetics (DESIGN.md sections 5.6, 7c).  fp16c: no bound can be derived
-- a short prefix averages the roundings of fewer tokens, which is why the mode has a length switch -- so each point is held to
max(2 x the error of the plain fp16c forward of the batch truncated at that point, 1e-4), that forward being existing code on the
same handle with the short-read switch off; the factor 2 covers the different transform size and merge order.  The summary is a
discrete function of the trajectory: exact against tests/trajectory_reference.py, every field of every read."""
from __future__ import annotations

import io
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import trajectory_reference as TR
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
TOL = 1e-4
CASES = ("3x1", "2x128", "2x129", "2x130", "3x257", "5x300", "5x300s256", "6x300c4", "2x8193")


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0, head_scale=3.0)


def _engine(prec, sd, chunk=256):
    from chimeralm_amd.engine import Engine

    e = Engine("cuda:0", precision=prec, chunk_reads=chunk)
    e.load_state_dict(sd)
    if prec == "fp16c":
        e.set_f16c_min_len(1)                                   # the 16-bit kernels themselves at every length
    return e


def _request(S=128, summary=True):
    from chimeralm_amd.engine import TrajectoryRequest

    return TrajectoryRequest(stride=S, summary=summary)


def _run(e, ids, S, **kw):
    """(logits, trajectory [B, K, 2], summary int32 [B, 12]) of one forward, on the host."""
    logits, trj = e.forward(torch.from_numpy(ids).cuda(), trajectory=_request(S), **kw)
    torch.cuda.synchronize()
    h = trj.to_host(non_blocking=False)
    return logits.cpu().numpy(), h.logits.numpy(), h.summary.numpy()


# ------------------------------------------------------------------------------------------------ 1, 5: interior points, summary
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_interior_points_against_the_fp64_reference(built_lib, sd, prec):
    engines = {}
    for name in CASES:
        ids, S, chunk = TR.case(name)
        e = engines.get(chunk) or engines.setdefault(chunk, _engine(prec, sd, chunk))
        logits, traj, summary = _run(e, ids, S)
        ref = TR.case_reference(name)
        K = ref.shape[1]
        assert traj.shape == ref.shape and np.isfinite(traj).all()
        err = float(np.abs(traj[:, :K - 1] - ref[:, :K - 1]).max()) if K > 1 else 0.0
        last = float(np.abs(traj[:, K - 1] - ref[:, K - 1]).max())
        print(f"{prec} {name}: K = {K}, interior max |dlogit| {err:.2e} (bound {TOL:.0e}), last point {last:.2e}")
        assert np.array_equal(traj[:, K - 1], logits)           # the forward's own logits, bit for bit
        assert err <= TOL and last <= TOL
        TR.check_summary(summary, traj, ids, S)
    for e in engines.values():
        e.close()


# ------------------------------------------------------------------------------------------------ 2: fp16c
def test_fp16c_points_against_the_plain_forward_of_the_truncated_batch(built_lib, sd):
    engines = {}
    worst = 0.0
    for name in CASES[2:]:                                      # from 129 tokens up
        ids, S, chunk = TR.case(name)
        e = engines.get(chunk) or engines.setdefault(chunk, _engine("fp16c", sd, chunk))
        logits, traj, summary = _run(e, ids, S)
        ref = TR.case_reference(name)
        K = ref.shape[1]
        assert np.array_equal(traj[:, K - 1], logits) and np.isfinite(traj).all()
        case_worst = 0.0
        for k, n in enumerate(TR.points(ids.shape[1], S)[:-1]):
            assert e.effective_precision(n) == "fp16c"
            plain = e.forward(torch.from_numpy(np.ascontiguousarray(ids[:, :n])).cuda()).cpu().numpy()
            plain_err = float(np.abs(plain - ref[:, k]).max())
            err = float(np.abs(traj[:, k] - ref[:, k]).max())
            case_worst = max(case_worst, err / max(plain_err, 0.5 * TOL))
            assert err <= max(2 * plain_err, TOL), (name, k, n, err, plain_err)
        print(f"fp16c {name}: worst trajectory error / max(plain error, 5e-5) over {K - 1} interior points {case_worst:.2f} (bound 2)")
        worst = max(worst, case_worst)
        TR.check_summary(summary, traj, ids, S)
    print(f"fp16c: worst ratio {worst:.2f}")
    for e in engines.values():
        e.close()


# ------------------------------------------------------------------------------------------------ 3: underflow
UNDERFLOW_GAP = 110.0             # exp(x) is exactly 0 in fp32 below x = -103.98 (denormals included): beyond it, with a margin


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_a_peak_behind_the_prefix_does_not_underflow_it(built_lib, sd, prec):
    """`head.attention.2.weight` scaled until, in a read whose scores peak in its last tile, everything in the first tile lies more
    than 104 below that peak (so every read's scores span far more than 90): normalised by the read's global maximum, as
    head_tiles_kernel merges, the first point is exp(-110) / exp(-110) = 0 / 0 in fp32; the running maximum keeps it finite and right.

    Passes in both arithmetics on an MI355X.  (A milder scale is harder on the engine, not on the merge: at x 23.2 -- spans 100 ... 123,
    the first tile only 39.6 below the peak, the softmax not yet one-hot -- fp32 interior points were 1.27e-4 from fp64 and the forward's
    own logits, point K - 1, 1.26e-4; fp16x3 3.14e-5 and 2.81e-5.)"""
    ids, S, _ = TR.case("5x300")
    t64 = torch.from_numpy(ids.astype(np.int64))
    L = ids.shape[1]
    last_tile = (L - 1) // 128 * 128

    def scores_of(weights):
        trace = {}
        ho.forward(t64, weights, torch.float64, trace=trace)
        return trace["scores"].numpy()

    s0 = scores_of(sd)
    peaked = s0.argmax(1) >= last_tile                          # the batch first: a peak in the last tile of at least one read
    assert peaked.any(), s0.argmax(1)
    scale = UNDERFLOW_GAP / float((s0.max(1) - s0[:, :128].max(1))[peaked].max())
    hot = {k: v.clone() for k, v in sd.items()}
    key = [k for k in hot if k.endswith("head.attention.2.weight")]
    assert len(key) == 1
    hot[key[0]] *= scale
    s = scores_of(hot)
    below = s.max(1) - s[:, :128].max(1)
    assert ((s.max(1) - s.min(1)) > 90).all()
    assert ((s.argmax(1) >= last_tile) & (below > 104)).any(), (s.argmax(1), below)
    print(f"{prec}: scale {scale:.1f}, spans {np.round(s.max(1) - s.min(1), 1)}, peaks at {s.argmax(1)}, first tile below the peak by {np.round(below, 1)}")
    ref = TR.trajectory_fp64(ids, hot, S)
    e = _engine(prec, hot)
    logits, traj, summary = _run(e, ids, S)
    K = ref.shape[1]
    err = float(np.abs(traj[:, :K - 1] - ref[:, :K - 1]).max())
    print(f"{prec}: interior max |dlogit| {err:.2e} (bound {TOL:.0e}); the forward's own logits (point K - 1, not this code's) "
          f"{float(np.abs(logits - ref[:, K - 1]).max()):.2e}")
    assert np.isfinite(traj).all()
    assert np.array_equal(traj[:, K - 1], logits)
    TR.check_summary(summary, traj, ids, S)
    e.close()
    assert err <= TOL


# ------------------------------------------------------------------------------------------------ 4: invariants
@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16c", "fp16", "bf16"])
def test_a_request_changes_no_logit_and_two_runs_agree(built_lib, sd, prec):
    from chimeralm_amd.engine import AttentionRequest

    e = _engine(prec, sd, chunk=4)
    for L, prefixes in ((600, (0, 200, 599, 5, 0, 130)), (2500, (0, 1000, 2499))):
        ids = TR.padded_batch(L, prefixes, seed=L)
        t = torch.from_numpy(ids).cuda()
        plain = e.forward(t).cpu().numpy()
        l1, t1, s1 = _run(e, ids, 128)
        l2, t2, s2 = _run(e, ids, 128)
        assert np.array_equal(plain, l1) and np.array_equal(plain, l2) and np.array_equal(plain, e.forward(t).cpu().numpy())
        assert np.array_equal(t1, t2) and np.array_equal(s1, s2)
        assert np.array_equal(t1[:, -1], plain)                 # point K - 1 is the call's logits, bit for bit
        l3, att, trj = e.forward(t, attention=AttentionRequest(top_k=5), trajectory=_request(256, summary=False))   # both requests
        _, att_alone = e.forward(t, attention=AttentionRequest(top_k=5))
        torch.cuda.synchronize()
        assert np.array_equal(l3.cpu().numpy(), plain) and trj.summary is None
        assert np.array_equal(trj.logits.cpu().numpy()[:, -1], plain)
        for k, v in att.tensors().items():
            assert torch.equal(v, att_alone.tensors()[k]), k
        coarse = trj.logits.cpu().numpy()
        assert np.array_equal(coarse[:, :-1], t1[:, 1:coarse.shape[1] * 2 - 1:2])   # stride 256: every second point of stride 128
        TR.check_summary(s1, t1, ids, 128)
    e.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16c"])
def test_launch_counts_without_a_request_are_the_engines_own(built_lib, sd, prec):
    """Per-stage launch counts of a profiled forward (`clm_profile_read`): without a request what the engine launched before the
    trajectory existed, and the same with one (its kernels are no timed stage)."""
    e = _engine(prec, sd, chunk=4)
    ids = TR.padded_batch(600, (0, 200, 599, 5, 0, 130), seed=4)
    t = torch.from_numpy(ids).cuda()
    e.forward(t)                                                # filters, workspace, [PAD] table
    want = {"embed": 2, "short_long_conv": 8, "out_proj_ln2_mlp": 8, "head_mlp": 2}      # 6 reads = 2 chunks of at most 4
    for trajectory in (None, _request(128)):
        e.profile_enable(True)
        e.profile_read(reset=True)
        e.forward(t, trajectory=trajectory)
        got = {k: n for k, (ms, n) in e.profile_read(reset=True).items() if n}
        e.profile_enable(False)
        assert got == want, (trajectory, got)
    e.close()


def test_a_self_check_between_two_forwards_leaves_the_users_buffers_alone(built_lib, sd):
    from chimeralm_amd import lm

    model = lm.ChimeraLM.new(precision="fp16c", trajectory_stride=128)
    model.load_state_dict(sd, strict=True)
    model.eval()
    net = model.net
    a_ids = torch.from_numpy(TR.padded_batch(2500, (0, 900, 2499, 0, 17, 0), seed=8)).cuda()
    b_ids = torch.from_numpy(TR.padded_batch(2300, (5, 0, 0, 1200, 0, 2299), seed=9)).cuda()
    la = model(a_ids, None)                                     # first batch: the seeded samples and this batch's rows are checked
    trj_a = net.last_trajectory
    assert net.selfcheck_report.get("checks") == 1
    keep = {k: v.clone() for k, v in trj_a.tensors().items()}
    net._guard.recheck_next = True                                    # a check is due on the next batch (guard_due)
    lb = model(b_ids, None)
    trj_b = net.last_trajectory
    assert net.selfcheck_report.get("checks") == 2 and trj_b is not trj_a
    torch.cuda.synchronize()
    for k, v in trj_a.tensors().items():                        # batch A's buffers: still batch A's
        assert torch.equal(v, keep[k]), k
    eng = net.engine(a_ids.device)
    for ids, logits, trj in ((a_ids, la, trj_a), (b_ids, lb, trj_b)):   # and both hold what a forward of their batch alone gives
        l2, again = eng.forward(ids, trajectory=net.trajectory_request())
        assert torch.equal(l2, logits)
        for k, v in trj.tensors().items():
            assert torch.equal(v, again.tensors()[k]), k
    h = trj_b.to_host(non_blocking=False)
    TR.check_summary(h.summary.numpy(), h.logits.numpy(), b_ids.cpu().numpy(), 128)


def test_summary_of_a_non_finite_curve(built_lib, sd):
    """NaN in the output layer's bias: every logit of every point is NaN -- the record says so instead of naming a point."""
    bad = {k: v.clone() for k, v in sd.items()}
    key = [k for k in bad if k.endswith("head.output_layer.bias")]
    assert len(key) == 1
    bad[key[0]][1] = float("nan")
    ids, S, _ = TR.case("5x300")
    e = _engine("fp32", bad)
    logits, traj, summary = _run(e, ids, S)
    assert np.isnan(traj[:, :, 1]).all() and np.isfinite(traj[:, :, 0]).all()
    TR.check_summary(summary, traj, ids, S)
    f = dict(zip(TR.FIELDS, summary.T))
    assert (f["onset_k"] == -1).all() and (f["jump_k"] == -1).all() and (f["n_nonfinite"] == 3 - f["first_k"]).all() and (f["label"] == 0).all()
    e.close()


# ------------------------------------------------------------------------------------------------ 6: argument errors
def test_request_argument_errors(built_lib, sd):
    import ctypes as C

    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import EngineError

    e = _engine("fp32", sd)
    t = torch.from_numpy(TR.padded_batch(300, (0, 10), seed=1)).cuda()
    out = torch.empty((2, 2), dtype=torch.float32, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")

    def call(eng=e, L=300, **kw):
        c = N.ClmTrajOut()
        c.struct_size, c.stride, c.logits, c.point_stride = C.sizeof(N.ClmTrajOut), 128, buf.data_ptr(), 3
        for k, v in kw.items():
            setattr(c, k, v)
        return eng._lib.clm_forward_traj(eng._h, C.c_void_p(t.data_ptr()), N.DT_U8, t.stride(0), 2, L, C.c_void_p(out.data_ptr()), None,
                                         C.byref(c), None)

    for stride in (0, 64, 192, 4224, -128):
        assert call(stride=stride) == N.E_INVALID, stride                                # not a multiple of 128 in 128 ... 4096
    assert call(point_stride=2) == N.E_INVALID and b"point_stride" in e._lib.clm_last_error(e._h)   # K = 3
    assert call(struct_size=24) == N.E_INVALID and b"size" in e._lib.clm_last_error(e._h)
    assert call(logits=None) == N.E_INVALID
    e.debug_stop_after(1, 2)
    assert call() == N.E_UNSUPPORTED and b"debug stop" in e._lib.clm_last_error(e._h)
    e.debug_stop_after(-1, -1)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                                 # a refused call wrote nothing
    assert call() == N.OK and call(stride=256, point_stride=2) == N.OK and call(stride=4096, point_stride=1) == N.OK
    with pytest.raises(ValueError):
        e.forward_staged(0, 2, trajectory=_request())                                    # (no length)
    with pytest.raises(EngineError):
        e.forward_staged(0, 2, trajectory=_request(), length=300)                        # nothing staged
    e.close()
    long = _engine("fp32", sd)
    big = torch.full((1, 32900), 8, dtype=torch.uint8, device="cuda")
    c = N.ClmTrajOut()
    c.struct_size, c.stride, c.logits, c.point_stride = C.sizeof(N.ClmTrajOut), 4096, buf.data_ptr(), 16
    rc = long._lib.clm_forward_traj(long._h, C.c_void_p(big.data_ptr()), N.DT_U8, big.stride(0), 1, 32900, C.c_void_p(out.data_ptr()), None,
                                    C.byref(c), None)
    assert rc == N.E_UNSUPPORTED and b"32832" in long._lib.clm_last_error(long._h)        # L > ATTN_MAX_L
    long.close()


def test_the_unfused_exact_path_is_refused(built_lib, sd):
    """CLM_DEBUG is read when a handle is created: a child process, so that no other test sees the switch."""
    code = ("import sys, torch\n"
            f"sys.path[:0] = [{str(REPO)!r}, {str(REPO / 'tests')!r}]\n"
            "from oracle import hyena_oracle as ho\n"
            "from chimeralm_amd.engine import Engine, EngineError, TrajectoryRequest\n"
            "from chimeralm_amd import _native as N\n"
            "e = Engine('cuda:0', precision='fp32'); e.load_state_dict(ho.make_state_dict(0, head_scale=3.0))\n"
            "t = torch.full((2, 300), 8, dtype=torch.uint8, device='cuda')\n"
            "e.forward(t)\n"
            "try:\n"
            "    e.forward(t, trajectory=TrajectoryRequest())\n"
            "except EngineError as err:\n"
            "    assert err.code == N.E_UNSUPPORTED and 'unfused' in str(err), err\n"
            "    print('refused')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, CLM_DEBUG="unfused_fp32"),
                       cwd=str(REPO), timeout=600)
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ 7: end to end
def _weights_dir(tmp_path, sd):
    from safetensors.torch import save_file

    wdir = tmp_path / "weights"
    wdir.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items() if not (k.endswith(".3.freq") or k.endswith(".5.freq"))},
              str(wdir / "model.safetensors"))
    return wdir


def _check_trajectory_files(out: Path, rank_batches, stride, lengths=None):
    names = []
    for rk, b in rank_batches:
        txt = [ln.split("\t") for ln in (out / f"{rk}_{b}.txt").read_text().splitlines()]
        tsv = [ln.split("\t") for ln in (out / f"{rk}_{b}.traj.tsv").read_text().split("\n")[:-1]]
        z = np.load(io.BytesIO((out / f"{rk}_{b}.traj.npz").read_bytes()))
        assert [(x[0], x[1]) for x in tsv] == [(x[0], x[1]) for x in txt]        # one line per read, in file order, same labels
        assert z["names"].tolist() == [x[0] for x in tsv]
        traj, seen = z["traj"], z["bases_seen"]
        B, K = seen.shape
        assert traj.shape == (B, K, 2) and np.isfinite(traj).all() and (np.diff(seen, axis=1) >= 0).all()
        for i, x in enumerate(tsv):
            assert len(x) == 10
            label, n_bases, k_pts = int(x[1]), int(x[2]), int(x[3])
            first, onset, before, at = (int(v) for v in x[4:8])
            assert k_pts == K and seen[i, -1] == n_bases and label == int(traj[i, -1, 1] > traj[i, -1, 0])
            if lengths is not None:
                assert n_bases == min(lengths[x[0]], 32768)
            gap = traj[i, :, 1].astype(np.float64) - traj[i, :, 0].astype(np.float64)
            assert x[9] == f"{np.float32(gap[-1]):.7g}"
            assert 0 < first <= min(stride, n_bases) and first <= onset <= n_bases and onset in seen[i]
            ko = int(np.flatnonzero(seen[i] == onset)[-1])
            assert all(int(g > 0) == label for g in gap[ko:])                    # from the onset on the label holds
            kf = int(np.flatnonzero(seen[i] > 0)[0])                             # first_k: the first point that holds a base
            steps = [(1 if label else -1) * (gap[k] - gap[k - 1]) for k in range(kf + 1, K)]
            if steps:                                                            # the largest step towards the label, and where
                assert x[8] == f"{np.float32(max(steps)):.7g}" and (before, at) == (seen[i, kf + int(np.argmax(steps))], seen[i, kf + 1 + int(np.argmax(steps))])
            else:
                assert (before, at, x[8]) == (-1, -1, "0")
        names += [x[0] for x in tsv]
    return names


def test_predict_writes_trajectory_files(tmp_path, golden_dir, built_lib, sd):
    from typer.testing import CliRunner

    from chimeralm_amd import bam as bam_mod, tokenizer as T
    from chimeralm_amd.__main__ import app
    from chimeralm_amd.callbacks import resume_read_name

    wdir = _weights_dir(tmp_path, sd)
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
    outs = {}
    for name, extra in (("plain", ["--feeder", "native"]),
                        ("native", ["--feeder", "native", "--save-trajectory", "--trajectory-values"]),
                        ("python", ["--feeder", "python", "--trajectory-values", "--save-attention"])):
        outs[name] = tmp_path / name
        r = CliRunner().invoke(app, ["predict", str(bam), "-b", "12", "-o", str(outs[name]), "--weights", str(wdir), "--precision", "fp32",
                                     *extra])
        assert r.exit_code == 0, (name, r.output[-2000:], r.exception)
    txt = sorted(p.name for p in outs["plain"].glob("*.txt"))
    assert txt and sorted(p.name for p in outs["plain"].iterdir()) == txt                 # no flags: the prediction files alone
    for name in ("native", "python"):
        assert sorted(p.name for p in outs[name].glob("*.txt")) == txt                    # `filter`'s glob sees the predictions alone
        for f in txt:                                                                     # ... byte for byte those of a plain run
            assert (outs[name] / f).read_bytes() == (outs["plain"] / f).read_bytes(), (name, f)
    assert sorted(p.name for p in outs["native"].iterdir()) == sorted(
        txt + [f.replace(".txt", ".traj.tsv") for f in txt] + [f.replace(".txt", ".traj.npz") for f in txt])
    assert sorted(p.name for p in outs["python"].iterdir()) == sorted(
        txt + [f.replace(".txt", e) for f in txt for e in (".traj.tsv", ".traj.npz", ".attn.tsv")])
    for f in txt:                                                                         # the two feeders: the same trajectory files
        for ext in (".traj.tsv", ".traj.npz"):
            g = f.replace(".txt", ext)
            assert (outs["native"] / g).read_bytes() == (outs["python"] / g).read_bytes(), g
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam_mod.BamDataModule(tokenizer=tok, predict_data_path=bam, batch_size=12)
    dm.setup("predict")
    order, length = [], {}
    for batch in dm.predict_dataloader():
        for row, ids in zip(batch["id"], batch["input_ids"]):
            order.append(resume_read_name(row))
            length[order[-1]] = int((ids != 4).sum()) - 1                                 # bases: without [SEP]
    got = _check_trajectory_files(outs["native"], [(0, b) for b in range(len(txt))], 128, length)
    assert got == order                                                                   # lines in read order


def test_predict_two_ranks_write_their_own_trajectory_files(tmp_path, golden_dir, built_lib, sd):
    """`predict -g 2 --save-trajectory` with both ranks on the one GPU over gloo, as tests/test_gpu_multirank.py runs it."""
    wdir = _weights_dir(tmp_path, sd)
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
    env = dict(os.environ, PYTHONPATH=str(REPO), CLM_DIST_BACKEND="gloo", CLM_RANKS_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MASTER_PORT", None)
    out = tmp_path / "two"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "predict", str(bam), "-g", "2", "-b", "24", "-o", str(out),
                        "--weights", str(wdir), "--precision", "fp32", "--save-trajectory", "--trajectory-values",
                        "--trajectory-stride", "1024"], capture_output=True, text=True, env=env, cwd=str(REPO), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    txt = sorted(p.name for p in out.glob("*_*.txt"))
    assert {f.split("_")[0] for f in txt} == {"0", "1"}
    assert sorted(p.name for p in out.glob("*.traj.tsv")) == sorted(f.replace(".txt", ".traj.tsv") for f in txt)
    assert sorted(p.name for p in out.glob("*.traj.npz")) == sorted(f.replace(".txt", ".traj.npz") for f in txt)
    names = _check_trajectory_files(out, [tuple(int(v) for v in f[:-4].split("_")) for f in txt], 1024)
    assert len(names) == len(set(names)) == 100                 # every selected read of the BAM, once
