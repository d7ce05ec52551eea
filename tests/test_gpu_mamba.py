"""The Mamba nets on MI355X (csrc/mamba.hip through the clm_mamba_* C ABI) against the fp64 forward of tests/mamba_reference.py,
which tests/golden/mamba_golden.npz pins to the reference modules' own wrapper code."""
import numpy as np
import pytest
import torch

import mamba_reference as mr

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # logits, both precisions
TOL_REL = 1e-5             # intermediates, relative to their largest magnitude
NAMES = ["m_l1", "m_l63", "m_l64", "m_l65", "m_l777pad", "m_l4101", "m_l8193", "m_mask", "m_ds64",
         "s_l1", "s_l63", "s_l64", "s_l65", "s_l777pad", "s_l4101", "s_l8193"]
VARIANT = {0: "mamba", 1: "mambasp"}


def _model(variant, sd, prec, d_state=None, n_layers=None, max_len=None, d_model=None, expand=None):
    from chimeralm_amd import mamba

    d, nl, ds, ex, mml = mr.VARIANTS[variant]
    ds, nl, mml, d, ex = d_state or ds, n_layers or nl, max_len or mml, d_model or d, expand or ex
    if variant == "mamba":
        net = mamba.MambaSequenceClassification(vocab_size=12, embedding_dim=d, number_of_layers=nl, model_max_length=mml, dropout=0.1,
                                                number_of_classes=2, d_state=ds, expand=ex, precision=prec)
    else:
        net = mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=d, number_of_layers=nl, number_of_classes=2, dropout=0.2,
                                                  d_state=ds, expand=ex, precision=prec)
    net.load_state_dict(sd, strict=True)
    return net


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "mamba_golden.npz")


def _case(golden, name):
    var, seed, B, L, pads, d_state, masked = (int(v) for v in golden[f"{name}_meta"])
    variant = VARIANT[var]
    sd = mr.make_mamba_state_dict(variant, seed, d_state=d_state)
    return variant, sd, d_state, golden[f"{name}_ids"], golden[f"{name}_mask"] if masked else None


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_golden_cases(built_lib, golden, prec):
    worst = 0.0
    for name in NAMES:
        variant, sd, d_state, ids, mask = _case(golden, name)
        ref = mr.mamba_forward_fp64(variant, sd, ids, mask=mask, device="cuda").cpu().numpy()
        net = _model(variant, sd, prec, d_state=d_state)
        m = torch.from_numpy(mask).cuda() if mask is not None else None
        got = net(torch.from_numpy(ids).cuda(), m).cpu().numpy()
        err_g, err_r = np.abs(got - golden[f"{name}_logits"]).max(), np.abs(got - ref).max()
        print(f"{prec} {name}: |logits - golden| = {err_g:.2e}, |logits - fp64| = {err_r:.2e}")
        worst = max(worst, err_g, err_r)
        assert err_g < TOL and err_r < TOL, name
        net.close()
    print(f"{prec}: worst logit error {worst:.2e}")


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name", ["m_mask", "s_l777pad"])
def test_intermediates(built_lib, golden, prec, name):
    variant, sd, d_state, ids, mask = _case(golden, name)
    tr = {}
    mr.mamba_forward_fp64(variant, sd, ids, mask=mask, trace=tr, device="cuda")
    net = _model(variant, sd, prec, d_state=d_state)
    net(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda() if mask is not None else None)
    B, L = ids.shape
    d = mr.VARIANTS[variant][0]
    for key, shape in (("front", (B, L, d)), ("layer0", (B, L, d)), ("pooled", (B, d))):
        want = tr[key].cpu().numpy()
        got = net.debug_fetch(key, shape)
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"{prec} {name} {key}: relative error {rel:.2e}")
        assert rel < TOL_REL, key
    net.close()


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_dtypes_strides_and_determinism(built_lib, variant):
    sd = mr.make_mamba_state_dict(variant, 20, n_layers=2)
    B, L = 3, 200
    ids = mr.synthetic_ids(2000, B, L, pads=17)
    ref = mr.mamba_forward_fp64(variant, sd, ids, device="cuda").cpu().numpy()
    net = _model(variant, sd, "fp16x3", n_layers=2)
    outs = []
    for dtype in (torch.int64, torch.int32, torch.uint8):
        wide = torch.zeros((B, L + 13), dtype=dtype)            # a row stride that is not L
        wide[:, 5:5 + L] = torch.from_numpy(ids).to(dtype)
        x = wide.cuda()[:, 5:5 + L]
        assert x.stride(0) == L + 13
        outs.append(net(x).cpu().numpy())
        assert np.abs(outs[-1] - ref).max() < TOL, dtype
    assert all(np.array_equal(o, outs[0]) for o in outs)
    again = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    assert np.array_equal(again, outs[0])                         # bitwise
    net.close()


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_batch_rows_equal_reads_alone(built_lib, variant):
    """Rows 0-3 and 250 of a 256 x 8,193 batch (several chunks of reads: row 250 lies in the third) equal the same reads run alone,
    bit for bit; `mamba` with a mask, so that each chunk's mask rows are the ones its reads see."""
    sd = mr.make_mamba_state_dict(variant, 21)
    ids = torch.from_numpy(mr.synthetic_ids(2100, 8, 8193)).cuda()
    big = ids.repeat(32, 1)
    big[4:] = torch.roll(big[4:], 1, dims=0)
    mask = None
    if variant == "mamba":
        g = torch.Generator().manual_seed(2101)
        mask = (torch.rand(256, 8193, generator=g) > 0.1).float().cuda()
    net = _model(variant, sd, "fp16x3")
    full = net(big, mask).cpu().numpy()
    assert np.isfinite(full).all()
    from chimeralm_amd.mamba import MambaEngineError
    for tap in ("zx", "xc", "g", "ssq", "part"):                  # the workspace holds the last chunk only: its taps are refused
        with pytest.raises(MambaEngineError, match="ran in chunks of"):
            net.debug_fetch(tap, (1,))
    for r in (0, 1, 2, 3, 250):
        alone = net(big[r:r + 1], None if mask is None else mask[r:r + 1]).cpu().numpy()
        assert np.array_equal(alone[0], full[r]), r
    if mask is not None:
        assert np.abs(full[250] - net(big[250:251]).cpu().numpy()[0]).max() > 1e-3     # (the mask row mattered)
    net.close()


@pytest.mark.parametrize("variant,kw", [("mamba", dict(d_state=32)), ("mamba", dict(d_model=512)),
                                        ("mambasp", dict(d_model=256)), ("mambasp", dict(d_state=64, expand=2))])
def test_other_supported_shapes(built_lib, variant, kw):
    """Shapes the engine accepts beyond the two reference configs: one layer, fp32 and fp16x3, against the fp64 forward."""
    sd = mr.make_mamba_state_dict(variant, 29, n_layers=1, **kw)
    ids = mr.synthetic_ids(2900, 2, 150, pads=9)
    ref = mr.mamba_forward_fp64(variant, sd, ids, device="cuda").cpu().numpy()
    for prec in ("fp32", "fp16x3"):
        net = _model(variant, sd, prec, n_layers=1, **kw)
        got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
        err = np.abs(got - ref).max()
        print(f"{variant} {kw} {prec}: |logits - fp64| = {err:.2e}")
        assert err < TOL, (kw, prec)
        net.close()


def test_mask_routes_and_mambasp_ignores_it(built_lib, golden):
    variant, sd, d_state, ids, mask = _case(golden, "m_mask")
    net = _model(variant, sd, "fp32", d_state=d_state)
    x = torch.from_numpy(ids).cuda()
    masked = net(x, torch.from_numpy(mask).cuda()).cpu().numpy()
    plain = net(x).cpu().numpy()
    assert np.abs(masked - golden["m_mask_logits"]).max() < TOL
    assert np.abs(masked - plain).max() > 1e-2
    wide = torch.zeros((ids.shape[0], ids.shape[1] + 9))
    wide[:, :ids.shape[1]] = torch.from_numpy(mask)
    strided = net(x, wide.cuda()[:, :ids.shape[1]]).cpu().numpy()
    assert np.array_equal(strided, masked)
    net.close()
    sp_sd = mr.make_mamba_state_dict("mambasp", 22, n_layers=1)
    sp = _model("mambasp", sp_sd, "fp32", n_layers=1)
    y = torch.from_numpy(mr.synthetic_ids(2200, 2, 100)).cuda()
    assert np.array_equal(sp(y).cpu().numpy(), sp(y, torch.zeros(2, 100).cuda()).cpu().numpy())
    sp.close()


def test_errors(built_lib):
    sd = mr.make_mamba_state_dict("mamba", 23, n_layers=1)
    net = _model("mamba", sd, "fp32", n_layers=1)
    with pytest.raises(ValueError, match="model_max_length"):
        net(torch.full((1, 30001), 7, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="at least one token"):
        net(torch.zeros((0, 100), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        net(torch.full((2, 100), 7, dtype=torch.int64, device="cuda"), torch.ones(2, 99, device="cuda"))
    out = net(torch.full((1, 30000), 7, dtype=torch.int64, device="cuda"))      # exactly model_max_length is fine
    assert torch.isfinite(out).all()
    net.close()


def test_in_place_weight_change_is_picked_up(built_lib):
    sd = mr.make_mamba_state_dict("mambasp", 24, n_layers=2)
    net = _model("mambasp", sd, "fp16x3", n_layers=2)
    ids = mr.synthetic_ids(2400, 2, 300)
    x = torch.from_numpy(ids).cuda()
    before = net(x).cpu().numpy()
    with torch.no_grad():
        net.mamba_layers[1].A_log.add_(0.7)
        net.mamba_layers[0].out_proj.weight.mul_(-1.0)
    sd2 = {k: v.clone() for k, v in net.state_dict().items()}
    after = net(x).cpu().numpy()
    ref = mr.mamba_forward_fp64("mambasp", sd2, ids, device="cuda").cpu().numpy()
    assert np.abs(after - before).max() > 1e-2
    assert np.abs(after - ref).max() < TOL
    net.close()


def test_fp16x3_range_guard_and_nonfinite_rerun(built_lib, caplog):
    ids = mr.synthetic_ids(2500, 2, 300)
    x = torch.from_numpy(ids).cuda()
    # a projection weight beyond the packing's range: the exact-fp32 kernels from the start
    sd = mr.make_mamba_state_dict("mambasp", 25, n_layers=2)
    sd["mamba_layers.1.in_proj.weight"][5, 7] = 100.0
    ref = mr.mamba_forward_fp64("mambasp", sd, ids, device="cuda").cpu().numpy()
    net = _model("mambasp", sd, "fp16x3", n_layers=2)
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got = net(x).cpu().numpy()
    rep = net.precision_report
    assert rep["fallback"] is True and rep["fallback_precision"] == "fp32" and rep["max_abs_weight"] == 100.0
    assert any("exact-fp32" in r.getMessage() for r in caplog.records)
    assert np.abs(got - ref).max() < TOL * max(1.0, float(np.abs(ref).max()))
    net.close()
    # activations beyond fp16's range (an embedding scaled by 2^17): fp16x3 returns NaN, the batch is rerun on fp32
    sd = mr.make_mamba_state_dict("mambasp", 26, n_layers=2)
    sd["embedding.weight"] = sd["embedding.weight"] * 131072.0
    ref = mr.mamba_forward_fp64("mambasp", sd, ids, device="cuda").cpu().numpy()
    net = _model("mambasp", sd, "fp16x3", n_layers=2)
    caplog.clear()
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got = net(x).cpu().numpy()
    assert net.precision_report["fallback"] is False and net.precision_report["nonfinite_reruns"] == 1
    assert any("rerun on the exact-fp32 kernels" in r.getMessage() for r in caplog.records)
    assert np.isfinite(got).all()
    pooled = net.debug_fetch("pooled", (2, 512))             # from the exact-fp32 handle that produced the logits
    assert np.isfinite(pooled).all()
    err = np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max()))
    print(f"fp16x3 rerun on fp32 with |E| up to {float(sd['embedding.weight'].abs().max()):.3g}: relative logit error {err:.2e}")
    assert err < TOL
    net.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("k", [8, 16])
def test_small_activations(built_lib, prec, k):
    """The low side of fp16x3's activation range: the weights and reads of the 2^17 case above with `embedding.weight` x 2^-k.  An
    unscaled fp16 split keeps an absolute 2^-25 of an activation below ~2^-3, and the RMS scale behind out_proj turns that back into
    a relative error (tests/error_model.py x3_linear; tests/test_mamba_stage_host.py holds the CPU model of exactly these nets:
    6.3e-5 at 2^-8, 2.3e-4 at 2^-16).  Both precisions are held to TOL of fp64, relative to max(1, max|ref|)."""
    ids = mr.synthetic_ids(2500, 2, 300)
    sd = mr.make_mamba_state_dict("mambasp", 26, n_layers=2)
    sd["embedding.weight"] = sd["embedding.weight"] * 2.0 ** -k
    ref = mr.mamba_forward_fp64("mambasp", sd, ids, device="cuda").cpu().numpy()
    net = _model("mambasp", sd, prec, n_layers=2)
    got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    err = np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max()))
    print(f"SMALL {prec} embedding x 2^-{k}: relative logit error {err:.2e} (|ref| up to {np.abs(ref).max():.2f}); report {net.precision_report}")
    net.close()
    assert err < TOL


@pytest.mark.parametrize("variant,L", [("mamba", 30000), ("mambasp", 32769)])
def test_longest_reads(built_lib, variant, L):
    sd = mr.make_mamba_state_dict(variant, 27)
    ids = mr.synthetic_ids(2700, 4, L, pads=100)
    net = _model(variant, sd, "fp16x3")
    got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    ref = mr.mamba_forward_fp64(variant, sd, ids[:2], device="cuda").cpu().numpy()
    err = np.abs(got[:2] - ref).max()
    print(f"{variant} 4 x {L}: |logits - fp64| = {err:.2e} on rows 0-1")
    assert err < TOL
    net.close()


@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_eval_py_route(tmp_path, golden_dir, built_lib, variant):
    """`python eval.py ckpt_path=... model=mamba|mambasp +data.predict_data_path=...` with a Lightning-layout checkpoint writes the
    files the same model gives through the Python API on the same batches.  The BAM route pads a batch to 32,769 tokens, so the
    `mamba` checkpoint here has a positional table of that length (model.net.model_max_length=32769)."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    from chimeralm_amd import bam, tokenizer as T
    from chimeralm_amd.basic_module import ClassificationLit
    from oracle import data_oracle as do

    repo = Path(__file__).resolve().parent.parent
    max_len = 32769 if variant == "mamba" else None
    sd = {f"net.{k}": v for k, v in mr.make_mamba_state_dict(variant, 28, model_max_length=max_len).items()}
    ckpt = tmp_path / f"{variant}.ckpt"
    torch.save({"state_dict": sd}, ckpt)
    out = tmp_path / "run"
    env = {**os.environ, "PYTHONPATH": str(repo)}
    r = subprocess.run([sys.executable, str(repo / "eval.py"), f"ckpt_path={ckpt}", f"model={variant}",
                        f"+data.predict_data_path={golden_dir / 'test_chimric_reads.bam'}", "data.batch_size=10",
                        "+data.max_predict_samples=20", "model.net.precision=fp32", f"hydra.run.dir={out}"]
                       + ([f"model.net.model_max_length={max_len}"] if max_len else []),
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted((out / "predicts").glob("*.txt"))
    assert [f.name for f in files] == ["0_0.txt", "0_1.txt"]
    net = _model(variant, mr.make_mamba_state_dict(variant, 0, model_max_length=max_len), "fp32", max_len=max_len)
    model = ClassificationLit(net).load_reference_checkpoint(ckpt)
    tok = T.load_tokenizer_from_hyena_model("hyenadna-small-32k-seqlen")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / "test_chimric_reads.bam", batch_size=10,
                           max_predict_samples=20)
    dm.setup("predict")
    for f, batch in zip(files, dm.predict_dataloader()):
        logits, _ = model.predict_step({**batch, "input_ids": batch["input_ids"].cuda()}, 0)
        assert f.read_text() == "".join(do.prediction_lines(logits.cpu().numpy(), batch["id"].numpy()))
