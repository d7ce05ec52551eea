"""Length-bucketed predict on MI355X (csrc/bucket.hip through the clm_bucket_* C ABI, chimeralm_amd/bucket.py, the `predict
--batching bucket` and `eval.py +batching.mode=bucket` routes): the scatter kernel byte for byte against numpy, the invariance of a
read's logits to batch size, read order and rank count -- bitwise for the Mamba and transformer nets, to the arithmetic's rounding
(1e-4 of the fp64 oracle, DESIGN.md sections 5.6 and 7c) for Hyena -- and both entry points on the reference's BAM.

Measured on an MI355X (worst |logit - fp64 oracle| over the 40 reads and four settings): fp32 1.6e-5, fp16x3 1.2e-5; in `file` mode the
same reads differ by up to 5.9 in a logit between batch 3 and batch 7."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import mamba_reference as mr
from oracle import hyena_oracle as ho
from test_bucket_host import _round16, model_length
from test_gpu_explain import SMALL_SP, _close, _hyena, _mamba, _net
from test_gpu_multirank import _free_port

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
BAM = "test_chimric_reads.bam"
PAD, SEP = 4, 1
HYENA_SEED = 2                      # of oracle.hyena_oracle.make_state_dict(head_scale=3.0): chosen on the CPU, see `oracle_logits`
LOGIT_TOL = 1e-4                    # fp32 and fp16x3 against the fp64 oracle (DESIGN.md sections 5.6, 7c)
MARGIN = 2e-3                       # labels are compared where the oracle's |logit1 - logit0| exceeds it


@pytest.fixture(scope="module")
def kernel(built_lib):
    from chimeralm_amd.bucket import Scatter

    h = Scatter("cuda:0")
    yield h
    h.close()


def _read(rng, n):
    """A read of n tokens: n - 1 seeded bases (A, C, G, T) and [SEP]."""
    return np.concatenate([7 + rng.integers(0, 4, size=n - 1), [SEP]]).astype(np.uint8)


def _left_padded(reads, L=None, stride=None, fill=0xEE):
    """(buffer [B, stride] with `fill` behind the columns, its [B, L] view): the reads padded on the left to L."""
    L = L if L is not None else max(len(r) for r in reads)
    buf = np.full((len(reads), stride if stride is not None else _round16(L)), fill, dtype=np.uint8)
    buf[:, :L] = PAD
    for i, r in enumerate(reads):
        buf[i, L - len(r): L] = r
    return buf, buf[:, :L]


def bucket_row(read):
    lc = model_length(len(read))
    return np.concatenate([np.full(lc - len(read), PAD, np.uint8), read])


# ------------------------------------------------------------------------------------------------ 1: the kernel alone
SLOTS = 6                                                                        # rows per class slab in the kernel tests
CLASSES = (65, 129, 257)
SLAB = {65: 0, 129: SLOTS * 80, 257: SLOTS * (80 + 144)}                         # slab offsets: strides 80, 144, 272
POOL_BYTES = SLOTS * (80 + 144 + 272)


def _spans(ns, L):
    """One span per row r: its n tokens into the smallest of the three classes that holds them, slot r + 1 (never slot 0)."""
    from chimeralm_amd.bucket import SPAN_DTYPE

    spans = np.zeros(len(ns), dtype=SPAN_DTYPE)
    for r, n in enumerate(ns):
        w = next(c for c in CLASSES if c >= n)
        spans[r] = (r, L - n, n, w, SLAB[w] + (r + 1) * _round16(w))
    return spans


def _np_pool(view, spans):
    pool = np.full(POOL_BYTES, 0xEE, dtype=np.uint8)
    for r, col, n, w, off in spans.tolist():
        pool[off: off + _round16(w)] = 0                                         # the tail behind the row, up to a multiple of 16
        pool[off: off + w - n] = PAD
        pool[off + w - n: off + w] = view[r, col: col + n]
    return pool


def test_scatter_bytes_equal_numpy(kernel):
    rng = np.random.default_rng(3)
    residues, last_byte = set(), False
    for L in range(193, 209):                                                    # stride round16(L) = 208: every source start mod 16
        menu = [1, 2, 15, 16, 17, 64, 65, 66, 129, L]
        menu = menu[L % 10:] + menu[: L % 10]                                    # every n comes by every row, the last included
        for ns in (menu[:5], menu[5:]):
            reads = [_read(rng, n) for n in ns]
            buf, view = _left_padded(reads, L)
            assert buf.shape == (5, 208)
            spans = _spans(ns, L)
            d_buf = torch.from_numpy(buf).cuda()
            pool = torch.full((POOL_BYTES,), 0xEE, dtype=torch.uint8, device="cuda")
            kernel.scatter(d_buf[:, :L], spans, 0, 5, pool)
            got = pool.cpu().numpy()
            want = _np_pool(view, spans)
            assert np.array_equal(got, want), (L, ns, np.flatnonzero(got != want)[:8])
            residues |= {(int(s["src_row"]) * 208 + int(s["src_col"])) % 16 for s in spans}
            last_byte |= L == 208                                                # row 4 then ends on the buffer's last byte
            assert {int(s["dst_width"]) for s in spans} <= set(CLASSES)
            for s0, rows in ((1, 3), (4, 1)):                                    # a part of the spans: only their rows are written
                pool.fill_(0xEE)
                kernel.scatter(d_buf[:, :L], spans, s0, rows, pool)
                assert np.array_equal(pool.cpu().numpy(), _np_pool(view, spans[s0: s0 + rows])), (L, ns, s0)
    assert residues == set(range(16)) and last_byte


def test_scatter_at_the_products_size(kernel):
    """Rows of 32,769 tokens (128 x 16 + 1 chunks: more than one block per row) next to a short one, through the planner."""
    from chimeralm_amd import bucket as B

    rng = np.random.default_rng(4)
    reads = [_read(rng, n) for n in (32769, 30000, 600, 32768)]
    buf, view = _left_padded(reads)
    planner = B.Planner(2)
    steps, spans, _ = planner.push([len(r) for r in reads], view.shape[1])
    fin, _, _ = planner.finish()
    planner.close()
    size = B.pool_bytes(2)
    pool = torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda")
    d_buf = torch.from_numpy(buf).cuda()
    want = np.full(size, 0xEE, dtype=np.uint8)
    emits = []
    for st in steps.tolist() + fin.tolist():
        kind, first, count, length, offset, stride = st
        if kind == 0:
            kernel.scatter(d_buf[:, : view.shape[1]], spans, first, count, pool)
            for r, col, n, w, off in spans[first: first + count].tolist():
                want[off: off + _round16(w)] = 0
                want[off: off + w] = bucket_row(reads[r])
        else:
            emits.append((length, count))
    assert np.array_equal(pool.cpu().numpy(), want)
    assert emits == [(32769, 2), (641, 1), (30721, 1)]                           # the full class at once, the rest in ascending length


def test_scatter_refuses_bad_arguments(kernel):
    rng = np.random.default_rng(5)
    ns = [3, 40, 200]
    buf, view = _left_padded([_read(rng, n) for n in ns], 200)
    spans = _spans(ns, 200)
    d_buf = torch.from_numpy(buf).cuda()
    d_ids = d_buf[:, :200]
    pool = torch.full((POOL_BYTES + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    odd = torch.zeros((3, 216), dtype=torch.uint8, device="cuda")[:, :200]       # a row stride that is no multiple of 16
    flat = torch.zeros((3 * 208 + 16,), dtype=torch.uint8, device="cuda")
    big = torch.full((POOL_BYTES + 32784,), 0xEE, dtype=torch.uint8, device="cuda")      # room for a row of 32,770: only its width is wrong

    def changed(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s

    cases = {
        "misaligned ids": lambda: kernel.scatter(flat[1: 1 + 3 * 208].view(3, 208)[:, :200], spans, 0, 3, pool[:POOL_BYTES]),
        "source stride": lambda: kernel.scatter(odd, spans, 0, 3, pool[:POOL_BYTES]),
        "misaligned pool": lambda: kernel.scatter(d_ids, spans, 0, 3, pool[1: 1 + POOL_BYTES]),
        "a span behind the pool": lambda: kernel.scatter(d_ids, changed(dst_offset=POOL_BYTES - 64), 0, 3, pool[:POOL_BYTES]),
        "a span before the pool": lambda: kernel.scatter(d_ids, changed(dst_offset=-16), 0, 3, pool[:POOL_BYTES]),
        "an offset that is no multiple of 16": lambda: kernel.scatter(d_ids, changed(dst_offset=8), 0, 3, pool[:POOL_BYTES]),
        "a span behind its source row": lambda: kernel.scatter(d_ids, changed(src_col=161), 0, 3, pool[:POOL_BYTES]),
        "a source row outside the batch": lambda: kernel.scatter(d_ids, changed(src_row=3), 0, 3, pool[:POOL_BYTES]),
        "more bytes than the row is wide": lambda: kernel.scatter(d_ids, changed(dst_width=39), 0, 3, pool[:POOL_BYTES]),
        "no bytes": lambda: kernel.scatter(d_ids, changed(n_copy=0), 0, 3, pool[:POOL_BYTES]),
        "rows > 65535": lambda: kernel.scatter(d_ids, np.tile(spans[:1], 65536), 0, 65536, pool[:POOL_BYTES]),   # 65,536 good spans
        "a row wider than 32769": lambda: kernel.scatter(d_ids, changed(dst_width=32770), 0, 3, big),
        "no rows": lambda: kernel.scatter(d_ids, spans, 0, 0, pool[:POOL_BYTES]),
        "s0 + rows > n_spans": lambda: kernel.scatter(d_ids, spans, 1, 3, pool[:POOL_BYTES]),
        "s0 < 0": lambda: kernel.scatter(d_ids, spans, -1, 1, pool[:POOL_BYTES]),
    }
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert (pool == 0xEE).all() and (big == 0xEE).all(), "a refused call launched"
    kernel.scatter(d_ids, np.tile(spans[:1], 65535), 0, 65535, pool[:POOL_BYTES])        # the limit itself is taken (sixteen launches)
    torch.cuda.synchronize()
    pool.fill_(0xEE)
    kernel.scatter(d_ids, spans, 0, 3, pool[:POOL_BYTES])                        # the same arguments, in order
    assert np.array_equal(pool[:POOL_BYTES].cpu().numpy(), _np_pool(view, spans)) and (pool[POOL_BYTES:] == 0xEE).all()


# ------------------------------------------------------------------------------------------------ 2: invariance
N_READS = 40


def make_reads(seed=7):
    """40 seeded reads of 1 ... 700 tokens, the extremes and a class top among them."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 701, size=N_READS)
    n[:4] = [1, 2, 65, 700]
    return [_read(rng, int(k)) for k in n]


def _staged(reads, index, batch_size):
    """File-order batches of `batch_size` of the reads `index`, padded on the left to their longest, as the loops stage them."""
    for i in range(0, len(index), batch_size):
        mine = index[i: i + batch_size]
        buf, view = _left_padded([reads[j] for j in mine], fill=0)
        L = view.shape[1]
        yield {"input_ids": torch.from_numpy(buf).cuda()[:, :L], "id": np.asarray(mine, dtype=np.int64)[:, None],
               "labels": np.asarray(mine, dtype=np.int64), "lengths": np.asarray([len(reads[j]) for j in mine], dtype=np.int32)}


def _bucketed(net, reads, index, batch_size):
    """{read: logits} of the reads `index` through `regroup` at `batch_size`; the id rows and labels must follow their reads."""
    from chimeralm_amd import bucket as B

    rg = B.Regrouper("cuda:0", batch_size)
    out = {}
    try:
        for batch in B.regroup(_staged(reads, index, batch_size), rg):
            ids = batch["input_ids"]
            rows = ids.cpu().numpy()
            logits = net(ids, None).cpu().numpy()
            which = batch["labels"].tolist()
            assert batch["id"][:, 0].tolist() == which and 1 <= len(which) <= batch_size and logits.shape == (len(which), 2)
            for k, j in enumerate(which):
                assert j not in out and np.array_equal(rows[k], bucket_row(reads[j])), j      # the row is a function of the read
                out[j] = logits[k]
        assert rg.n_rows == len(index) and rg.n_tokens == sum(model_length(len(reads[j])) for j in index)
    finally:
        rg.close()
    assert sorted(out) == sorted(index)
    return out


def _settings(net, reads):
    """The four settings: batch size 3 and 7, the reads shuffled, and the reads split r::2 as two ranks would; [40, 2] each."""
    order = list(range(N_READS))
    shuffled = np.random.default_rng(11).permutation(N_READS).tolist()
    runs = {"batch 3": _bucketed(net, reads, order, 3), "batch 7": _bucketed(net, reads, order, 7),
            "shuffled": _bucketed(net, reads, shuffled, 3),
            "two ranks": {**_bucketed(net, reads, order[0::2], 3), **_bucketed(net, reads, order[1::2], 3)}}
    return {k: np.stack([v[j] for j in order]) for k, v in runs.items()}


def _file_mode(net, reads, batch_size):
    out = np.zeros((N_READS, 2), dtype=np.float32)
    for batch in _staged(reads, list(range(N_READS)), batch_size):
        out[batch["labels"]] = net(batch["input_ids"], None).cpu().numpy()
    return out


@pytest.mark.parametrize("name", ["mambasp", "transformer"])
def test_logits_bitwise_invariant(built_lib, name):
    reads = make_reads()
    net = _mamba("mambasp", 0, "fp16x3", **{**SMALL_SP, "n_layers": 2}) if name == "mambasp" else _net("transformer")
    try:
        got = _settings(net, reads)
        alone = np.stack([net(torch.from_numpy(bucket_row(r)).cuda().view(1, -1), None).cpu().numpy()[0] for r in reads])
        assert np.isfinite(alone).all()
        for setting, logits in got.items():
            assert np.array_equal(logits.view(np.int32), alone.view(np.int32)), (name, setting)
    finally:
        _close(net)


@pytest.fixture(scope="module")
def oracle_logits():
    """The fp64 oracle's forward of every read's bucket row alone ([40, 2]); rows of one length go through it together (its rows do
    not see each other).  HYENA_SEED was picked on the CPU so that the oracle's own margins leave at most 10 % of the reads under
    the label rule: with seed 2 the oracle labels 20 of the 40 reads 1 and its smallest margin is 0.128 (seeds 0, 1 and 3 give
    all reads one label)."""
    reads = make_reads()
    sd = ho.make_state_dict(HYENA_SEED, head_scale=3.0)
    rows = [bucket_row(r) for r in reads]
    out = np.zeros((N_READS, 2))
    for lc in sorted({len(x) for x in rows}):
        idx = [i for i, x in enumerate(rows) if len(x) == lc]
        out[idx] = ho.forward(torch.from_numpy(np.stack([rows[i] for i in idx]).astype(np.int64)), sd, dt=torch.float64).numpy()
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_hyena_within_rounding_of_the_oracle(built_lib, oracle_logits, prec):
    """Hyena packs two reads into one transform: a row is independent of its partner up to rounding only, so the logits are held to
    the fp64 oracle of the read's bucket row alone (1e-4), and two settings differ by at most 2e-4."""
    reads = make_reads()
    margin = np.abs(oracle_logits[:, 1] - oracle_logits[:, 0])
    decided = margin > MARGIN
    assert (~decided).sum() <= N_READS // 10                                     # the oracle alone: at most 10 % under the rule
    net = _hyena(HYENA_SEED, prec)
    try:
        got = _settings(net, reads)
        worst = {k: float(np.abs(v - oracle_logits).max()) for k, v in got.items()}
        print(f"hyena {prec}: worst |logit - fp64 oracle| per setting {worst}")
        for setting, logits in got.items():
            assert worst[setting] <= LOGIT_TOL, (prec, setting, worst)
            assert np.array_equal((logits[:, 1] > logits[:, 0])[decided], (oracle_logits[:, 1] > oracle_logits[:, 0])[decided]), setting
        a, b = _file_mode(net, reads, 3), _file_mode(net, reads, 7)
        print(f"hyena {prec}: file mode, batch 3 against batch 7: worst |dlogit| {float(np.abs(a - b).max()):.3e}")
        assert np.abs(a - b).max() > 2 * LOGIT_TOL                               # the problem being fixed: a read's logits follow its batch
    finally:
        _close(net)


# ------------------------------------------------------------------------------------------------ 3: end to end
def _names(d):
    files = sorted(Path(d).glob("*_*.txt"))
    return [ln.split("\t")[0] for f in files for ln in f.read_text().splitlines()], files


@pytest.fixture(scope="module")
def weights_dir(tmp_path_factory):
    from safetensors.torch import save_file

    sd = ho.make_state_dict(0, head_scale=3.0)
    wdir = tmp_path_factory.mktemp("bucket_weights")
    save_file({k: v.contiguous() for k, v in sd.items() if not (k.endswith(".3.freq") or k.endswith(".5.freq"))},
              str(wdir / "model.safetensors"))
    return wdir


@pytest.fixture(scope="module")
def file_mode_names(built_lib, golden_dir, tmp_path_factory):
    """The names `file` mode writes for the fixture (one in-process pass of the native loop)."""
    from chimeralm_amd import lm, predict as loop
    from chimeralm_amd.callbacks import PredictionWriter
    from chimeralm_amd.feeder import BamFeeder

    model = lm.ChimeraLM.new(precision="fp16x3", selfcheck=False)
    model.load_state_dict(ho.make_state_dict(0, head_scale=3.0), strict=True)
    d = tmp_path_factory.mktemp("bucket_file_mode")
    try:
        with BamFeeder(golden_dir / BAM, batch_size=12) as fd:
            assert loop.run_predict_native(model, fd, PredictionWriter(d), torch.device("cuda", 0)) == 100
    finally:
        _close(model.net)
    names, files = _names(d)
    assert len(names) == len(set(names)) == 100 and len(files) == 9
    return set(names)


def test_cli_predict_bucket_and_filter(built_lib, golden_dir, tmp_path, weights_dir, file_mode_names):
    from chimeralm_amd import bucket as B
    from chimeralm_amd.filter import filter_bam_by_predcition
    from test_longread_host import _fixture_lengths

    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / BAM, bam)
    out = tmp_path / "pred"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "predict", str(bam), "-b", "12", "-o", str(out), "--weights", str(weights_dir),
                        "--precision", "fp16x3", "--batching", "bucket"],
                       capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(REPO), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names, files = _names(out)
    assert len(names) == 100 and set(names) == file_mode_names
    lc = [B.canonical_length(min(int(n), 32768) + 1) for n in _fixture_lengths(golden_dir)]
    n_batches = sum(-(-lc.count(c) // 12) for c in set(lc))                      # no class of the fixture reaches 12 reads: one file per class
    assert sorted(f.name for f in files) == sorted(f"0_{k}.txt" for k in range(n_batches)) and n_batches == 39
    assert "963,236 tokens forwarded" in r.stderr + r.stdout
    res = filter_bam_by_predcition(bam, out, index=True)
    assert res and res["kept"] + res["dropped"] > 0


def test_eval_py_bucket_mambasp(built_lib, golden_dir, tmp_path, file_mode_names):
    from chimeralm_amd import bucket as B
    from test_longread_host import _fixture_lengths

    sd = {"net." + k: v for k, v in mr.make_mamba_state_dict("mambasp", 0, **SMALL_SP).items()}
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, str(REPO / "eval.py"), f"ckpt_path={ckpt}", "model=mambasp",
                        f"+data.predict_data_path={golden_dir / BAM}", "+batching.mode=bucket", "data.batch_size=8", f"hydra.run.dir={out}",
                        "model.net.embedding_dim=256", "model.net.number_of_layers=1", "model.net.d_state=16", "model.net.expand=2"],
                       capture_output=True, text=True, env={**os.environ, "PYTHONPATH": str(REPO)}, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names, files = _names(out / "predicts")
    lc = [B.canonical_length(min(int(n), 32768) + 1) for n in _fixture_lengths(golden_dir)]
    n_batches = sum(-(-lc.count(c) // 8) for c in set(lc))                       # 39 classes; the one of 12 reads fills once at batch 8
    assert len(names) == 100 and set(names) == file_mode_names and len(files) == n_batches == 40


def test_two_ranks_each_name_once(built_lib, golden_dir, tmp_path, weights_dir, file_mode_names):
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / BAM, bam)
    env = dict(os.environ, PYTHONPATH=str(REPO), CLM_DIST_BACKEND="gloo", CLM_RANKS_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               MASTER_PORT=str(_free_port()))
    out = tmp_path / "two"
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "predict", str(bam), "-g", "2", "-b", "24", "-o", str(out),
                        "--weights", str(weights_dir), "--precision", "fp16x3", "--batching", "bucket"],
                       capture_output=True, text=True, env=env, cwd=str(REPO), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names, files = _names(out)
    assert len(names) == len(set(names)) == 100 and set(names) == file_mode_names      # each name once across the ranks
    ranks = {f.name.split("_")[0] for f in files}
    assert ranks == {"0", "1"}
    for rk in ranks:                                                             # a rank's files are its batches 0 ... k - 1
        mine = sorted(int(f.stem.split("_")[1]) for f in files if f.name.startswith(rk + "_"))
        assert mine == list(range(len(mine)))
