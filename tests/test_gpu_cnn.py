"""DNAConvNet on MI355X (csrc/cnn.hip + tail32.hip through the clm_cnn_* C ABI) against the fp64 forward of tests/cnn_reference.py,
which tests/golden/cnn_golden.npz pins to the reference module itself."""
import numpy as np
import pytest
import torch

import cnn_reference as cr

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # logits, both precisions (measured errors are ~1e-5)
TOL_REL = 1e-5             # intermediates, relative to their largest magnitude
CASES = ["l64", "l65", "l777pad", "l4101", "l8193"]


def _model(sd, prec):
    from chimeralm_amd.cnn import DNAConvNet

    net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                     hidden_dim=512, number_of_classes=2, dropout=0.1, precision=prec)
    net.load_state_dict(sd, strict=True)
    return net


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "cnn_golden.npz")


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases(built_lib, golden, prec, name):
    seed, B, L, pads = (int(v) for v in golden[f"{name}_meta"])
    sd = cr.make_cnn_state_dict(seed)
    ids = golden[f"{name}_ids"]
    ref = cr.cnn_forward_fp64(sd, ids).numpy()
    assert np.abs(ref - golden[f"{name}_logits"]).max() < 1e-4
    net = _model(sd, prec)
    got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    err_g, err_r = np.abs(got - golden[f"{name}_logits"]).max(), np.abs(got - ref).max()
    print(f"{prec} {name}: |logits - golden| = {err_g:.2e}, |logits - fp64| = {err_r:.2e}")
    assert err_g < TOL and err_r < TOL
    net.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("B,L", [(1, 64), (3, 65), (1, 127), (3, 2055), (1, 32770)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.uint8])
def test_shapes_dtypes_and_strides(built_lib, prec, B, L, dtype):
    sd = cr.make_cnn_state_dict(5)
    ids = cr.synthetic_ids(500 + L, B, L, pads=L // 10)
    ref = cr.cnn_forward_fp64(sd, ids).numpy()
    net = _model(sd, prec)
    wide = torch.zeros((B, L + 13), dtype=dtype)            # a row stride that is not L
    wide[:, 5:5 + L] = torch.from_numpy(ids).to(dtype)
    x = wide.cuda()[:, 5:5 + L]
    assert x.stride(0) == L + 13
    got = net(x).cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{prec} {dtype} B={B} L={L}: |logits - fp64| = {err:.2e}")
    assert np.isfinite(got).all() and err < TOL
    net.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_intermediates(built_lib, prec):
    sd = cr.make_cnn_state_dict(6)
    B, L = 2, 3001
    ids = cr.synthetic_ids(600, B, L, pads=33)
    tr = {}
    cr.cnn_forward_fp64(sd, ids, trace=tr)
    net = _model(sd, prec)
    net(torch.from_numpy(ids).cuda())
    for name, shape in (("block0", (B, L // 4, 256)), ("block1", (B, L // 16, 256)), ("pooled", (B, 256))):
        got, ref = net.debug_fetch(name, shape), tr[name].numpy()
        rel = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{prec} {name}: relative error {rel:.2e}")
        assert rel < TOL_REL, f"{prec} {name}: {rel:.2e}"
    net.close()


def test_determinism_and_batch_independence(built_lib):
    sd = cr.make_cnn_state_dict(7)
    B, L = 256, 8193
    ids = torch.from_numpy(cr.synthetic_ids(700, B, L)).cuda()
    for prec in ("fp32", "fp16x3"):
        net = _model(sd, prec)
        a = net(ids).cpu()
        b = net(ids).cpu()
        assert torch.equal(a, b), prec
        assert torch.isfinite(a).all()
        four = net(ids[:4].contiguous()).cpu()
        assert torch.equal(a[:4], four), prec
        ref = cr.cnn_forward_fp64(sd, ids[:4].cpu().numpy()).float()
        err = float((four - ref).abs().max())
        print(f"{prec} 256 x 8193: rows 0-3 bitwise equal to a batch of 4, |logits - fp64| = {err:.2e}")
        assert err < TOL
        net.close()


def test_errors(built_lib):
    from chimeralm_amd.cnn import CnnEngineError

    sd = cr.make_cnn_state_dict(0)
    net = _model(sd, "fp32")
    with pytest.raises(CnnEngineError, match="at least 64 tokens"):
        net(torch.full((2, 63), 7, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.full((2, 100), 7, dtype=torch.int64))
    net.close()


def test_out_of_range_ids_are_clamped(built_lib):
    sd = cr.make_cnn_state_dict(8)
    ids = cr.synthetic_ids(800, 2, 300)
    bad = ids.copy()
    bad[0, 10], bad[1, 200] = 200, 11 + 50            # clamped to the last row of the table, id 11
    ids[0, 10], ids[1, 200] = 11, 11
    net = _model(sd, "fp32")
    got = net(torch.from_numpy(bad).cuda()).cpu().numpy()
    ref = cr.cnn_forward_fp64(sd, ids).numpy()
    assert np.abs(got - ref).max() < TOL
    net.close()


def test_in_place_weight_change_is_picked_up(built_lib):
    sd = cr.make_cnn_state_dict(9)
    ids = cr.synthetic_ids(900, 2, 500)
    net = _model(sd, "fp16x3")
    x = torch.from_numpy(ids).cuda()
    before = net(x).cpu().numpy()
    with torch.no_grad():
        net.conv_blocks[1][0].weight.mul_(-1.0)
        net.fc[1].running_var.add_(0.5)
    sd2 = {k: v.clone() for k, v in net.state_dict().items()}
    after = net(x).cpu().numpy()
    ref = cr.cnn_forward_fp64(sd2, ids).numpy()
    assert np.abs(after - before).max() > 1e-2
    assert np.abs(after - ref).max() < TOL
    net.close()


def test_fp16x3_range_guard_falls_back_to_fp32(built_lib, caplog):
    sd = cr.make_cnn_state_dict(10)
    sd["conv_blocks.1.0.weight"][3, 17, 2] = 100.0
    ids = cr.synthetic_ids(1000, 2, 400)
    ref = cr.cnn_forward_fp64(sd, ids).numpy()
    net = _model(sd, "fp16x3")
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    rep = net.precision_report
    assert rep["fallback"] is True and rep["fallback_precision"] == "fp32" and rep["max_abs_weight"] == 100.0
    assert any("exact-fp32" in r.getMessage() for r in caplog.records)
    err = np.abs(got - ref).max()
    print(f"fp16x3 with |w| = 100 (exact-fp32 kernels): |logits - fp64| = {err:.2e} at logits up to {np.abs(ref).max():.1f}")
    assert err < TOL * max(1.0, float(np.abs(ref).max()))
    net.close()
    ok = _model(cr.make_cnn_state_dict(10), "fp16x3")
    ok(torch.from_numpy(ids).cuda())
    assert ok.precision_report["fallback"] is False
    ok.close()


def test_eval_py_cnn_route(tmp_path, golden_dir, built_lib):
    """`python eval.py ckpt_path=... model=cnn +data.predict_data_path=...` with a Lightning-layout DNAConvNet checkpoint writes the
    files the same model gives through the Python API on the same batches."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    from chimeralm_amd import bam, tokenizer as T
    from chimeralm_amd.basic_module import ClassificationLit
    from oracle import data_oracle as do

    repo = Path(__file__).resolve().parent.parent
    sd = {f"net.{k}": v for k, v in cr.make_cnn_state_dict(11).items()}
    ckpt = tmp_path / "cnn.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "run"
    env = {**os.environ, "PYTHONPATH": str(repo)}
    r = subprocess.run([sys.executable, str(repo / "eval.py"), f"ckpt_path={ckpt}", "model=cnn",
                        f"+data.predict_data_path={golden_dir / 'test_chimric_reads.bam'}", "data.batch_size=10",
                        "+data.max_predict_samples=20", "model.net.precision=fp32", f"hydra.run.dir={out}"],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted((out / "predicts").glob("*.txt"))
    assert [f.name for f in files] == ["0_0.txt", "0_1.txt"]
    model = ClassificationLit(_model(cr.make_cnn_state_dict(0), "fp32")).load_reference_checkpoint(ckpt)
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / "test_chimric_reads.bam", batch_size=10,
                           max_predict_samples=20)
    dm.setup("predict")
    for f, batch in zip(files, dm.predict_dataloader()):
        logits, _ = model.predict_step({**batch, "input_ids": batch["input_ids"].cuda()}, 0)
        assert f.read_text() == "".join(do.prediction_lines(logits.cpu().numpy(), batch["id"].numpy()))
