"""GPU (MI355X): attention as an output of the Hyena engine (csrc/attn_weights.hip, clm_forward_attn; DESIGN.md "Attention as an
output").

Bounds.  For a softmax, log w_i = s_i - logsumexp(s) and |d logsumexp| <= max |ds|, so scores that differ by at most ds give weights
with |d log w_i| <= 2 ds.  The kernel's own error -- the fp32 exp of an argument of up to ~20 (the subtraction s - max rounds to
20 x 2^-24 = 1.2e-6, exp itself to 1-2 ulp) and a sum carried in fp64 -- is below 1e-5 relative.  So:
  kernel alone     |log(w / w64)| <= 1e-5 wherever w64 >= 1e-30, w64 = the fp64 softmax of the scores of the SAME forward
  against another arithmetic (the oracle, an fp32 engine)   |log(w / w_ref)| <= 2 ds + 1e-5 with ds measured in the same test
Peaks and the integer summary fields are exact functions of the kernel's own weights and ids (tests/attn_reference.py)."""
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

from attn_reference import check_against, softmax64, summarize
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
KERNEL_TOL = 1e-5
PRECISIONS = ("fp32", "fp16x3", "fp16c", "fp16", "bf16")


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


def _padded_batch(L, prefixes, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(7, 11, size=(len(prefixes), L)).astype(np.uint8)
    ids[:, -1] = 1                                              # [SEP]
    for b, p in enumerate(prefixes):
        ids[b, :p] = 4
    return ids


def _request(top_k=10, weights=True):
    from chimeralm_amd.engine import AttentionRequest

    return AttentionRequest(top_k=top_k, weights=weights)


def _host(att):
    torch.cuda.synchronize()
    return att.to_host(non_blocking=False)


def _log_ratio(w, ref):
    """max |log(w / ref)| where ref >= 1e-30 (fp64)."""
    ref = np.asarray(ref, np.float64)
    m = ref >= 1e-30
    assert m.any() and (np.asarray(w)[m] > 0).all()
    return float(np.abs(np.log(np.asarray(w, np.float64)[m] / ref[m])).max())


# ------------------------------------------------------------------------------------------------ 1: the kernel alone
def _small_batch(L):
    if L == 1:
        return np.array([[1], [4], [8]], np.uint8)              # [SEP] alone, [PAD] alone, one base without [SEP]
    if L == 2:
        return np.array([[4, 1], [9, 1], [4, 4], [7, 8]], np.uint8)
    return _padded_batch(L, {257: (0, 3, 255, 256), 1025: (0, 1024, 300), 8193: (0, 8000, 127), 32769: (0, 20000)}[L], seed=L)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_kernel_against_fp64_softmax_of_its_own_scores(built_lib, sd, prec):
    e = _engine(prec, sd)
    for L in (1, 2, 257, 1025, 8193, 32769):
        ids = _small_batch(L)
        B = len(ids)
        top_k = 32 if L == 257 else 10
        logits, att = e.forward(torch.from_numpy(ids).cuda(), attention=_request(top_k))
        a = _host(att)
        scores = e.debug_fetch("scores", (B, L))                # one chunk: the scores of this very forward
        w, w64 = a.weights.numpy(), softmax64(scores)
        err, rowsum = _log_ratio(w, w64), float(np.abs(w.astype(np.float64).sum(1) - 1).max())
        print(f"{prec} {B} x {L}: max |log(w / w64)| {err:.2e}, max |row sum - 1| {rowsum:.2e}, |scores| <= {np.abs(scores).max():.3g}")
        assert np.isfinite(scores).all() and np.isfinite(logits.cpu().numpy()).all()
        assert err <= KERNEL_TOL and rowsum <= KERNEL_TOL
        check_against(a, ids, top_k, rel=KERNEL_TOL)
    e.close()


# ------------------------------------------------------------------------------------------------ 2: against the oracle
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_weights_against_the_oracle(built_lib, sd, prec):
    e = _engine(prec, sd, chunk=8)
    first, _ = ho.synthetic_batch(5, 3, 256, seed=99)           # the batch of test_gpu_parity.test_intermediates_fp32
    first[:, :4] = 4
    batches = [first, _padded_batch(700, (0, 1, 127, 128, 129, 500, 699), seed=1200),      # test_gpu_pad_prefix's prefixes: rows from
               _padded_batch(1025, (1024, 0, 256, 300, 1000), seed=1525),                  # the [PAD] table, the peeled last token
               _padded_batch(3000, (2944, 2000, 0, 2943), seed=3500)]
    for ids in batches:
        B, L = ids.shape
        trace = {}
        ho.forward(torch.from_numpy(ids.astype(np.int64)), sd, trace=trace)
        _, att = e.forward(torch.from_numpy(ids).cuda(), attention=_request(10))
        a = _host(att)
        s_ref = trace["scores"].numpy().reshape(B, L)
        w_ref = trace["attn_weights"].numpy().reshape(B, L)
        ds = float(np.abs(e.debug_fetch("scores", (B, L)) - s_ref).max())
        bound_s = 2e-5 * float(np.abs(s_ref).max()) + 1e-6
        err = _log_ratio(a.weights.numpy(), w_ref)
        print(f"{prec} {B} x {L}: score error {ds:.2e} (bound {bound_s:.2e}), max |log(w / w_ref)| {err:.2e} (bound {2 * ds + 1e-5:.2e})")
        assert ds <= bound_s
        assert err <= 2 * ds + 1e-5
        check_against(a, ids, 10, rel=KERNEL_TOL)
    e.close()


# ------------------------------------------------------------------------------------------------ 3: chunks
@pytest.mark.parametrize("prec", ["fp32", "fp16c"])
def test_a_batch_of_three_chunks_is_its_chunks(built_lib, sd, prec):
    L = 700
    ids = _padded_batch(L, (0, 300, 1, 128, 699, 0, 500, 129, 40, 256), seed=31)
    e = _engine(prec, sd, chunk=4)
    t = torch.from_numpy(ids).cuda()
    logits, att = e.forward(t, attention=_request(10))
    whole = _host(att)
    logits = logits.cpu()
    for lo, hi in ((0, 4), (4, 8), (8, 10)):
        l2, a2 = e.forward(t[lo:hi].contiguous(), attention=_request(10))
        part = _host(a2)
        assert torch.equal(l2.cpu(), logits[lo:hi])
        for k, v in part.tensors().items():
            assert torch.equal(v, whole.tensors()[k][lo:hi]), (k, lo)
    check_against(whole, ids, 10, rel=KERNEL_TOL)
    e.close()


def test_save_attention_covers_every_chunk(built_lib, sd):
    """`head.save_attention` (the reference's knob, hyena.py:129-130): a CPU tensor [B, L, 1] whose EVERY row is that read's weights
    -- with B > chunk_reads the debug tap it was built on held the last chunk only."""
    from chimeralm_amd import lm

    L = 700
    ids = _padded_batch(L, (0, 300, 1, 128, 699, 0, 500, 129, 40, 256), seed=31)
    model = lm.ChimeraLM.new(save_attention=True, precision="fp32", chunk_reads=4)
    model.load_state_dict(sd, strict=True)
    model.eval()
    logits = model(torch.from_numpy(ids).cuda(), None)
    w = model.net.head.attention_weights
    assert w.shape == (10, L, 1) and w.dtype == torch.float32 and w.device.type == "cpu"
    assert model.net.last_attention is None                     # (attention_top_k was not set)
    e = _engine("fp32", sd, chunk=4)
    l2, att = e.forward(torch.from_numpy(ids).cuda(), attention=_request(None, True))
    assert torch.equal(l2.cpu(), logits.cpu())
    assert torch.equal(_host(att).weights, w[..., 0])           # the same kernel, the same arithmetic: the same bits
    trace = {}
    ho.forward(torch.from_numpy(ids.astype(np.int64)), sd, trace=trace)
    for b in range(10):                                         # every row, the first chunk's included
        assert _log_ratio(w[b, :, 0].numpy(), trace["attn_weights"][b, :, 0].numpy()) <= 1e-3, b
    e.close()


# ------------------------------------------------------------------------------------------------ 4: no side effects
@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_request_changes_no_logit_and_two_runs_agree(built_lib, sd, prec):
    e = _engine(prec, sd, chunk=4)
    for L, prefixes in ((600, (0, 200, 599, 5, 0, 130)), (2500, (0, 1000, 2499))):
        t = torch.from_numpy(_padded_batch(L, prefixes, seed=L)).cuda()
        plain = e.forward(t).cpu()
        l1, a1 = e.forward(t, attention=_request(7))
        a1 = _host(a1)
        l2, a2 = e.forward(t, attention=_request(7))
        a2 = _host(a2)
        l3, a3 = e.forward(t, attention=_request(7, weights=False))      # peaks only: the same peaks
        a3 = _host(a3)
        assert torch.equal(plain, l1.cpu()) and torch.equal(plain, l2.cpu()) and torch.equal(plain, l3.cpu())
        assert torch.equal(plain, e.forward(t).cpu())
        for k, v in a1.tensors().items():
            assert torch.equal(v, a2.tensors()[k]), k
        assert a3.weights is None
        for k, v in a3.tensors().items():
            assert torch.equal(v, a1.tensors()[k]), k
    e.close()


def test_request_argument_errors(built_lib, sd):
    import ctypes as C

    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import EngineError

    e = _engine("fp32", sd)
    t = torch.from_numpy(_padded_batch(300, (0, 10), seed=1)).cuda()
    out = torch.empty((2, 2), dtype=torch.float32, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")

    def call(**kw):
        c = N.ClmAttnOut()
        c.struct_size = C.sizeof(N.ClmAttnOut)
        for k, v in kw.items():
            setattr(c, k, v)
        return e._lib.clm_forward_attn(e._h, C.c_void_p(t.data_ptr()), N.DT_U8, t.stride(0), 2, 300, C.c_void_p(out.data_ptr()),
                                       C.byref(c), None)

    p = buf.data_ptr()
    assert call() == N.E_INVALID                                                         # asks for nothing
    assert call(weights=p, weights_row_stride=299) == N.E_INVALID                        # rows would overlap
    assert call(summary=p, peak_pos=p + 4096, top_k=10) == N.E_INVALID                   # peak_weight missing
    assert call(summary=p, peak_pos=p + 4096, peak_weight=p + 8192, top_k=0) == N.E_INVALID
    assert call(summary=p, peak_pos=p + 4096, peak_weight=p + 8192, top_k=33) == N.E_INVALID
    assert call(struct_size=8, weights=p, weights_row_stride=300) == N.E_INVALID
    assert b"top_k" in e._lib.clm_last_error(e._h) or b"size" in e._lib.clm_last_error(e._h)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                                 # a refused call wrote nothing
    with pytest.raises(ValueError):
        e.forward_staged(0, 2, attention=_request())                                     # (no length)
    with pytest.raises(EngineError):
        e.forward_staged(0, 2, attention=_request(), length=300)                         # nothing staged
    e.close()


def test_a_self_check_between_two_forwards_leaves_the_users_buffers_alone(built_lib, sd):
    from chimeralm_amd import lm

    model = lm.ChimeraLM.new(precision="fp16c", attention_top_k=5)
    model.load_state_dict(sd, strict=True)
    model.eval()
    net = model.net
    net.attention_device_weights = True
    a_ids = torch.from_numpy(_padded_batch(2500, (0, 900, 2499, 0, 17, 0), seed=8)).cuda()
    b_ids = torch.from_numpy(_padded_batch(2300, (5, 0, 0, 1200, 0, 2299), seed=9)).cuda()
    la = model(a_ids, None)                                     # first batch: the seeded samples and this batch's rows are checked
    att_a = net.last_attention
    assert net.selfcheck_report.get("checks") == 1
    keep = {k: v.clone() for k, v in att_a.tensors().items()}
    net._guard.recheck_next = True                                    # a check is due on the next batch (guard_due)
    lb = model(b_ids, None)
    att_b = net.last_attention
    assert net.selfcheck_report.get("checks") == 2 and att_b is not att_a
    torch.cuda.synchronize()
    for k, v in att_a.tensors().items():                        # batch A's buffers: still batch A's
        assert torch.equal(v, keep[k]), k
    eng = net.engine(a_ids.device)
    for ids, logits, att in ((a_ids, la, att_a), (b_ids, lb, att_b)):   # and both hold what a forward of their batch alone gives
        l2, again = eng.forward(ids, attention=net.attention_request())
        assert torch.equal(l2, logits)
        for k, v in att.tensors().items():
            assert torch.equal(v, again.tensors()[k]), k
    check_against(_host(att_b), b_ids.cpu().numpy(), 5, rel=KERNEL_TOL)


@pytest.mark.parametrize("prec", ["fp32", "fp16c"])
def test_launch_counts_without_a_request_are_the_engines_own(built_lib, sd, prec):
    """Per-stage launch counts of a profiled forward (`clm_profile_read`): without a request what the engine launched before the
    attention output existed -- one embedding, four convolutions, four fused tails (block 0 reads the id table: no in_proj) and
    the head, per chunk -- and the same with one (its kernel is no timed stage)."""
    e = _engine(prec, sd, chunk=4)
    t = torch.from_numpy(_padded_batch(600, (0, 200, 599, 5, 0, 130), seed=4)).cuda()
    e.forward(t)                                                # filters, workspace, [PAD] table
    want = {"embed": 2, "short_long_conv": 8, "out_proj_ln2_mlp": 8, "head_mlp": 2}      # 6 reads = 2 chunks of at most 4
    for attention in (None, _request(10)):
        e.profile_enable(True)
        e.profile_read(reset=True)
        e.forward(t, attention=attention)
        got = {k: n for k, (ms, n) in e.profile_read(reset=True).items() if n}
        e.profile_enable(False)
        assert got == want, (attention, got)
    e.close()


# ------------------------------------------------------------------------------------------------ 5: size
@pytest.mark.parametrize("B,L", [(256, 8193), (32, 32769)])
def test_bench_size_batches_against_an_fp32_engine(built_lib, sd, B, L):
    from chimeralm_amd.hyena import HyenaDna

    rng = np.random.default_rng(L)
    ids = _padded_batch(L, [0 if b % 3 else int(rng.integers(1, L - 100)) for b in range(B)], seed=B)
    e = _engine("fp16c", sd)
    logits, att = e.forward(torch.from_numpy(ids).cuda(), attention=_request(10))
    a = _host(att)
    scores = e.debug_fetch("scores", (B, L))                    # (one chunk at both sizes)
    f = {k: v.numpy() for k, v in a.fields().items()}
    w = a.weights.numpy()
    assert np.isfinite(w).all() and np.isfinite(logits.cpu().numpy()).all()
    assert all(np.isfinite(f[k]).all() for k in ("pad_weight", "sep_weight", "base_weight"))
    assert (f["n_pad"] + f["n_bases"] + f["has_sep"] == L).all() and (f["has_sep"] == 1).all()
    assert (f["n_peaks"] == np.minimum(10, f["n_bases"])).all()
    assert np.abs(f["pad_weight"] + f["sep_weight"] + f["base_weight"] - 1).max() <= 1e-5
    pos, pw = a.peak_pos.numpy(), a.peak_weight.numpy()
    assert (pos >= 0).all() and (pos < f["n_bases"][:, None]).all() and (np.diff(pw, axis=1) <= 0).all()
    rows = HyenaDna._sample_rows(B, 4)
    ref = _engine("fp32", sd)
    _, att32 = ref.forward(torch.from_numpy(ids[rows]).cuda(), attention=_request(10))
    w32 = _host(att32).weights.numpy()
    s32 = ref.debug_fetch("scores", (len(rows), L))
    for i, b in enumerate(rows):
        ds = float(np.abs(scores[b] - s32[i]).max())
        err = _log_ratio(w[b], w32[i].astype(np.float64))
        print(f"fp16c {B} x {L} row {b}: score difference from fp32 {ds:.2e}, max |log(w / w32)| {err:.2e} (bound {2 * ds + 1e-5:.2e})")
        assert err <= 2 * ds + 1e-5
        r = summarize(w[b], ids[b], 10)
        assert pos[b].tolist() == r["pos"] and int(f["n_pad"][b]) == r["n_pad"]
    e.close(), ref.close()


# ------------------------------------------------------------------------------------------------ 6: end to end
def _weights_dir(tmp_path, sd):
    from safetensors.torch import save_file

    wdir = tmp_path / "weights"
    wdir.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items() if not (k.endswith(".3.freq") or k.endswith(".5.freq"))},
              str(wdir / "model.safetensors"))
    return wdir


def _check_attention_files(out: Path, rank_batches, reads_in_order=None, top_k=10):
    names = []
    for rk, b in rank_batches:
        txt = [ln.split("\t") for ln in (out / f"{rk}_{b}.txt").read_text().splitlines()]
        tsv = [ln.split("\t") for ln in (out / f"{rk}_{b}.attn.tsv").read_text().split("\n")[:-1]]
        z = np.load(io.BytesIO((out / f"{rk}_{b}.attn.npz").read_bytes()))
        assert [(x[0], x[1]) for x in tsv] == [(x[0], x[1]) for x in txt]        # one line per read, in file order, same labels
        assert z["names"].tolist() == [x[0] for x in tsv] and z["offsets"][-1] == len(z["weights"])
        for i, x in enumerate(tsv):
            assert len(x) == 7
            n_bases, n_pad = int(x[2]), int(x[3])
            wb = z["weights"][z["offsets"][i]: z["offsets"][i + 1]]
            assert len(wb) == n_bases == int(z["n_bases"][i])
            if reads_in_order is not None:
                assert n_bases <= reads_in_order[x[0]]
            peaks = [(int(p), w) for p, w in (q.split(":") for q in x[6].split(";") if q)]
            assert len(peaks) == min(top_k, n_bases) and all(0 <= p < n_bases for p, _ in peaks)
            order = np.lexsort((np.arange(n_bases), -wb.astype(np.float64)))[:top_k]    # the npz weights re-derive the tsv peaks
            assert [p for p, _ in peaks] == order.tolist()
            assert [w for _, w in peaks] == [f"{wb[p]:.6g}" for p in order]
            assert 0 <= float(x[4]) <= 1 and 0 <= float(x[5]) <= 1
            assert abs(float(x[4]) + float(x[5]) + float(wb.astype(np.float64).sum()) - 1) <= 2e-5
        names += [x[0] for x in tsv]
    return names


def test_predict_writes_attention_files(tmp_path, golden_dir, built_lib, sd):
    from typer.testing import CliRunner

    from chimeralm_amd import bam as bam_mod, tokenizer as T
    from chimeralm_amd.__main__ import app
    from chimeralm_amd.callbacks import resume_read_name

    wdir = _weights_dir(tmp_path, sd)
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
    outs = {}
    for name, extra in (("plain", ["--feeder", "native"]),
                        ("native", ["--feeder", "native", "--save-attention", "--attention-weights"]),
                        ("python", ["--feeder", "python", "--save-attention", "--attention-weights"])):
        outs[name] = tmp_path / name
        r = CliRunner().invoke(app, ["predict", str(bam), "-b", "12", "-o", str(outs[name]), "--weights", str(wdir), "--precision", "fp32",
                                     *extra])
        assert r.exit_code == 0, (name, r.output[-2000:], r.exception)
    txt = sorted(p.name for p in outs["plain"].glob("*.txt"))
    assert txt and sorted(p.name for p in outs["plain"].iterdir()) == txt                 # no flags: the prediction files alone
    for name in ("native", "python"):
        assert sorted(p.name for p in outs[name].glob("*.txt")) == txt
        for f in txt:                                                                     # the .txt files: byte for byte those of a plain run
            assert (outs[name] / f).read_bytes() == (outs["plain"] / f).read_bytes(), (name, f)
        assert sorted(p.name for p in outs[name].iterdir()) == sorted(
            txt + [f.replace(".txt", ".attn.tsv") for f in txt] + [f.replace(".txt", ".attn.npz") for f in txt])
    for f in txt:                                                                         # the two feeders: the same attention files
        for ext in (".attn.tsv", ".attn.npz"):
            g = f.replace(".txt", ext)
            assert (outs["native"] / g).read_bytes() == (outs["python"] / g).read_bytes(), g
    # the reads in file order with their lengths, from the Python data module
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam_mod.BamDataModule(tokenizer=tok, predict_data_path=bam, batch_size=12)
    dm.setup("predict")
    order, length = [], {}
    for batch in dm.predict_dataloader():
        for row, ids in zip(batch["id"], batch["input_ids"]):
            order.append(resume_read_name(row))
            length[order[-1]] = int((ids != 4).sum())
    got = _check_attention_files(outs["native"], [(0, b) for b in range(len(txt))], length)
    assert got == order


def test_predict_two_ranks_write_their_own_attention_files(tmp_path, golden_dir, built_lib, sd):
    """`predict -g 2 --save-attention` with both ranks on the one GPU over gloo, as tests/test_gpu_multirank.py runs it."""
    wdir = _weights_dir(tmp_path, sd)
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
    env = dict(os.environ, PYTHONPATH=str(REPO), CLM_DIST_BACKEND="gloo", CLM_RANKS_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MASTER_PORT", None)
    out = tmp_path / "two"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "predict", str(bam), "-g", "2", "-b", "24", "-o", str(out),
                        "--weights", str(wdir), "--precision", "fp32", "--save-attention", "--attention-weights",
                        "--attention-top-k", "3"], capture_output=True, text=True, env=env, cwd=str(REPO), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    txt = sorted(p.name for p in out.glob("*_*.txt"))
    assert {f.split("_")[0] for f in txt} == {"0", "1"}
    assert sorted(p.name for p in out.glob("*.attn.tsv")) == sorted(f.replace(".txt", ".attn.tsv") for f in txt)
    assert sorted(p.name for p in out.glob("*.attn.npz")) == sorted(f.replace(".txt", ".attn.npz") for f in txt)
    names = _check_attention_files(out, [tuple(int(v) for v in f[:-4].split("_")) for f in txt], top_k=3)
    assert len(names) == len(set(names)) == 100                 # every selected read of the BAM, once
