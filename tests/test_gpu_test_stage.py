"""GPU (one MI355X): the labelled test stage end to end, `python eval.py ckpt_path=... data=fq model=<net> data.batch_size=12
data.test_data_path=tests.parquet` (25 labelled reads, three batches), for three of the nets behind the `net` boundary.

This checks the stage, not the forward (which has its own parity tests): the metrics must be what plain torch computes on the host,
in float64, from the logits `model.predict_step` returns for the same batches -- counts equal, losses within 1e-12 relative (the
kernel works in double from the same fp32 logits; only exp / log rounding and the order of 25 additions differ).

The checkpoints are seeded, and the bias of the last layer is then shifted by the median logit difference over the 25 reads, so
that about half of them are predicted as each class: without both classes F1, precision and recall would say nothing.

The two-rank runs put both ranks on this one GPU over gloo, as tests/test_gpu_multirank.py does.  Their batches differ from the
one-rank run's (6 reads per rank and batch, other padding), so the yardstick is the host computation over the two ranks' own dumped
logits, not the one-rank metrics.  pyarrow is needed here and its absence is a failure."""
from __future__ import annotations

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from eval_reference import COUNTS, host_result

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
DRIVER = REPO / "tests" / "eval_stage_driver.py"
REL = 1e-12
NAMES = ("test/loss", "test/f1", "test/precision", "test/recall")
# net -> (seeded state_dict under the module's keys, key of the last layer's bias, extra overrides)
NETS = ("cnn", "mambasp", "hyena")


def _seeded(net: str) -> tuple[dict, str, list[str]]:
    if net == "cnn":
        import cnn_reference as cr

        return {f"net.{k}": v for k, v in cr.make_cnn_state_dict(5).items()}, "net.fc.4.bias", []
    if net == "mambasp":
        import mamba_reference as mr

        return {f"net.{k}": v for k, v in mr.make_mamba_state_dict("mambasp", 31).items()}, "net.classifier.3.bias", []
    from oracle import hyena_oracle as ho

    # (fp32: the 16-bit default would add its self-check's own state to what two runs must have in common)
    return ho.make_state_dict(0, head_scale=3.0), "net.head.output_layer.bias", ["model.net.precision=fp32"]


def _overrides(net: str, ckpt: Path, parquet: Path, extra: list[str]) -> list[str]:
    return [f"ckpt_path={ckpt}", "data=fq", f"model={net}", "data.batch_size=12", f"data.test_data_path={parquet}", *extra]


def _objects(overrides: list[str], tmp_path: Path):
    from chimeralm_amd.config import compose, instantiate

    cfg = compose(REPO / "configs", "eval.yaml", overrides, output_dir=tmp_path / "compose")
    return instantiate(cfg.model), instantiate(cfg.data)


def _logits(model, dm, world: int = 1, rank: int = 0) -> list[tuple[torch.Tensor, torch.Tensor]]:
    dm.setup("test", world_size=world, rank=rank)
    out = []
    with torch.inference_mode():
        for i, batch in enumerate(dm.test_dataloader()):
            logits, labels = model.predict_step({**batch, "input_ids": batch["input_ids"].to(torch.uint8).cuda()}, i)   # a byte per id, as the route
            out.append((logits.cpu(), labels))
    return out


def _checkpoint(net: str, tmp_path: Path, parquet: Path) -> tuple[Path, list[str]]:
    """A Lightning-layout checkpoint of seeded weights whose last bias splits the 25 reads between the classes."""
    sd, bias, extra = _seeded(net)
    ckpt = tmp_path / f"{net}.ckpt"
    model, dm = _objects(_overrides(net, ckpt, parquet, extra), tmp_path)
    model.load_state_dict(sd, strict=True)
    diff = torch.cat([lg[:, 1] - lg[:, 0] for lg, _ in _logits(model, dm)])
    assert diff.shape == (25,) and float(diff.max() - diff.min()) > 1e-4, "the seeded net gives every read the same logits"
    sd = dict(sd)
    sd[bias] = sd[bias].clone()
    sd[bias][1] -= diff.median()
    torch.save({"state_dict": sd}, ckpt)
    return ckpt, extra


def _env() -> dict:
    env = dict(os.environ, PYTHONPATH=str(REPO), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    return env


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _check_metrics(m: dict, want: dict, where: str):
    """`m`: the route's callback_metrics; `want`: the host sums over the same batches."""
    from chimeralm_amd.eval_metrics import metrics_from_result

    ref = metrics_from_result(want)
    print(where, {k: m[k] for k in NAMES + ("test/loss_per_read",)}, {k: m[f"test/{k}"] for k in ("tp", "fp", "tn", "fn")})
    assert set(NAMES) <= set(m)
    for k in COUNTS:
        assert m[f"test/{k}"] == want[k], (where, k)
    assert m["test/n_valid"] == 25 and m["test/n_invalid_labels"] == m["test/n_nonfinite"] == m["test/n_empty_batches"] == 0
    assert m["test/tp"] + m["test/fp"] > 0 and m["test/tn"] + m["test/fn"] > 0, "one class was never predicted: F1 says nothing"
    assert m["test/tp"] + m["test/fn"] == 14 and m["test/tn"] + m["test/fp"] == 11          # the labels of tests.parquet
    for k in ("test/f1", "test/precision", "test/recall"):
        assert m[k] == ref[k], (where, k)                      # the same double arithmetic on the same counts
    for k in ("test/loss", "test/loss_per_read"):
        print(f"    {k}: got {m[k]!r} want {ref[k]!r} rel {abs(m[k] - ref[k]) / abs(ref[k]):.3e}")
        assert abs(m[k] - ref[k]) <= REL * abs(ref[k]), (where, k)


@pytest.mark.parametrize("net", NETS)
def test_eval_py_test_route_equals_host_metrics(net, tmp_path, golden_dir, built_lib):
    import pyarrow  # noqa: F401 - the route needs it: fail here, do not skip

    parquet = golden_dir / "tests.parquet"
    ckpt, extra = _checkpoint(net, tmp_path, parquet)
    overrides = _overrides(net, ckpt, parquet, extra)
    out = tmp_path / "one"
    r = subprocess.run([sys.executable, str(DRIVER), str(out), *overrides, f"hydra.run.dir={tmp_path / 'run'}"],
                       capture_output=True, text=True, env=_env(), cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "test/f1" in r.stderr and "Test metrics (25 reads, 1 ranks)" in r.stderr          # rank 0 logs the table
    m = json.loads((out / "metrics0.json").read_text())
    model, dm = _objects(overrides, tmp_path)
    model.load_reference_checkpoint(ckpt)
    mine = _logits(model, dm)
    assert [lg.shape[0] for lg, _ in mine] == [12, 12, 1]
    _check_metrics(m, host_result(mine), net)
    assert m["test/n_batches"] == 3
    # what the kernel was given are those logits and labels, bit for bit
    dumped = torch.load(out / "rank0.pt")
    assert len(dumped) == 3 and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(dumped, mine))


@pytest.mark.parametrize("net", NETS)
def test_two_ranks_on_one_gpu_count_every_read_once(net, tmp_path, golden_dir, built_lib):
    import pyarrow  # noqa: F401

    parquet = golden_dir / "tests.parquet"
    ckpt, extra = _checkpoint(net, tmp_path, parquet)
    overrides = _overrides(net, ckpt, parquet, extra)
    out = tmp_path / "two"
    env = dict(_env(), CLM_DIST_BACKEND="gloo", CLM_RANKS_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(_free_port()), str(DRIVER), str(out), *overrides, "trainer=ddp",
                        f"hydra.run.dir={tmp_path / 'run'}"],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    dumps = [torch.load(out / f"rank{rk}.pt") for rk in (0, 1)]
    assert [[lg.shape[0] for lg, _ in d] for d in dumps] == [[6, 6, 1], [6, 6]]
    # rank r saw reads r, r + 2, ...: its labels are those rows' labels
    gold = json.loads((golden_dir / "eval_golden.json").read_text())["parquet"]["labels"]
    for rk in (0, 1):
        assert torch.cat([lb for _, lb in dumps[rk]]).tolist() == gold[rk::2]
    m0, m1 = (json.loads((out / f"metrics{rk}.json").read_text()) for rk in (0, 1))
    assert m0 == m1                                            # both ranks report the same merged metrics
    want = host_result(dumps[0] + dumps[1])                    # rank order, as the merge
    _check_metrics(m0, want, f"{net} x2")
    assert m0["test/n_batches"] == len(dumps[0]) + len(dumps[1]) == 5
    # the ranks' own batches through one process give the dumped logits (like for like: a batch's padding shows in its logits)
    model, dm = _objects(overrides, tmp_path)
    model.load_reference_checkpoint(ckpt)
    for rk in (0, 1):
        for (a, _), (b, _) in zip(_logits(model, dm, world=2, rank=rk), dumps[rk]):
            assert torch.equal(a, b), (net, rk)
