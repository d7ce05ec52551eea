"""GPU (MI355X): parity of the HIP engine, called through the C ABI, with the CPU oracle on the same seeded inputs.

The parity gate (north_star: identical labels, logits within 1e-3 of the fp32 reference) is GATE = 1e-3 and applies to the
two modes that claim reference parity:
  fp32   exact-fp32 MFMA                                   observed ~1e-5
  fp16c  fp16 activations x (hi + lo) fp16 weight pairs    observed 2-6e-4   <- the throughput mode (bench.py default)
  fp16x3 every operand as two halfs, three fp16 MFMAs      observed ~1e-5    (round 4: held to 1e-4, a tenth of the gate)
Labels must be identical on every row whose oracle margin exceeds 2 x GATE.
The plain 16-bit modes are REDUCED-PRECISION modes outside the gate; their bounds below only pin their rounding behaviour:
  fp16   |logit - oracle| <= 5e-3  (observed 0.5-1.5e-3), labels identical wherever the oracle margin > 2e-2
  bf16   |logit - oracle| <= 6e-2  (observed ~2e-2),       labels identical wherever the oracle margin > 2e-1
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import data_oracle as do
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent

GATE = 1e-3
TOL = {"fp32": GATE, "fp16c": GATE, "fp16x3": 1e-4, "fp16": 5e-3, "bf16": 6e-2}
MARGIN = {"fp32": 2 * GATE, "fp16c": 2 * GATE, "fp16x3": 2e-4, "fp16": 2e-2, "bf16": 2e-1}


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0, head_scale=3.0)


@pytest.fixture(scope="module")
def engines(sd, built_lib):
    from chimeralm_amd.engine import Engine

    out = {}
    for prec in ("fp32", "fp16c", "fp16", "bf16"):
        e = Engine("cuda:0", precision=prec, chunk_reads=4)
        e.load_state_dict(sd)
        out[prec] = e
    yield out
    for e in out.values():
        e.close()


def _ids(B, L, seed=5, pads=0):
    ids, _ = ho.synthetic_batch(seed, B, L - 1, seed=99)
    if pads:
        ids[:, :pads] = 4
    return ids


def _check(engine, prec, ids_np, sd, dtype=torch.int64, ref=None):
    if ref is None:
        ref = ho.forward(torch.from_numpy(ids_np.astype(np.int64)), sd).numpy()
    got = engine.forward(torch.from_numpy(ids_np).to(dtype).cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    assert err <= TOL[prec], f"{prec}: max |logit error| {err:.3e} > {TOL[prec]}"
    decided = np.abs(ref[:, 0] - ref[:, 1]) > MARGIN[prec]
    assert (got.argmax(1)[decided] == ref.argmax(1)[decided]).all()
    return err


@pytest.mark.parametrize("B,L", [(1, 2), (1, 5), (3, 129), (2, 128), (5, 300), (4, 513), (3, 1000), (7, 2049)])
def test_fp32_parity_shapes(engines, sd, B, L):
    """Odd batches (half-empty read pair), every FFT size class incl. the aliased L = N/2 + 1 cases."""
    _check(engines["fp32"], "fp32", _ids(B, L, pads=min(3, L - 1)), sd)


@pytest.mark.parametrize("prec", ["fp16c", "fp16", "bf16"])
@pytest.mark.parametrize("B,L", [(3, 129), (5, 300), (6, 1000)])
def test_16bit_modes(engines, sd, prec, B, L):
    _check(engines[prec], prec, _ids(B, L, pads=2), sd)


@pytest.mark.parametrize("B,L", [(1, 2), (1, 5), (2, 128), (4, 513), (3, 2047), (3, 2048), (7, 2049), (2, 4097)])
def test_fp16c_parity_shapes(engines, sd, B, L):
    """The throughput mode at the gate over the same shape classes as the fp32 mode.  Reads below 2048 tokens run through the
    fp16x3 kernels inside the fp16c engine (too few tokens for the pooling to average the fp16 activation roundings,
    clm_api.hip effective_prec); 2047 / 2048 straddle that switch and alternate the element type of the shared z / y buffers."""
    _check(engines["fp16c"], "fp16c", _ids(B, L, pads=min(3, L - 1)), sd)


@pytest.mark.parametrize("B,L", [(3, 130), (2, 257), (5, 300), (4, 513), (3, 1000), (2, 1500), (3, 2047)])
def test_fp16c_kernels_below_the_default_length_switch(sd, built_lib, B, L):
    """The guard may move the short-read switch down to 256 tokens when the loaded weights allow it, so the 16-bit kernels of fp16c --
    round 4: with the lo planes of y / z and the lo tiles of both LayerNorms -- must be RIGHT at those lengths too (one-shot
    convolution kernels of 256 .. 4096 points with lo bytes, partial last tiles whose rows beyond the read are masked, the peeled
    lone token at 257 / 513): forced with clm_set_short_read_len(1).  Their error grows like 1 / sqrt(L) (which is why the switch
    exists); round 3's mode measured 5.6e-4 at
    1,000 tokens and 1.5e-3 at 100."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=411, pads=2)
    ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sd).numpy()
    e = Engine("cuda:0", precision="fp16c", chunk_reads=4)
    e.load_state_dict(sd)
    e.set_f16c_min_len(1)
    assert e.effective_precision(L) == "fp16c"
    t = torch.from_numpy(ids).cuda()
    got = e.forward(t).cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"fp16c kernels at {B} x {L}: |logits - oracle| {err:.2e}")
    assert err <= GATE, err                                                      # measured 1.1e-4 (2,047 tokens) .. 5.3e-4 (257)
    assert np.array_equal(got, e.forward(t).cpu().numpy())                      # deterministic
    decided = np.abs(ref[:, 0] - ref[:, 1]) > 4e-3
    assert (got.argmax(1)[decided] == ref.argmax(1)[decided]).all()
    e.close()


# The UNGUARDED mode over the 32 batches of the study.  Round 3 (weights hi + lo only): worst 1.04e-3, 13 of 32 above the guard's
# 5e-4 -- the bound had to sit ABOVE the gate.  Round 4 (+ e5m2 lo bytes for y, the gated z rows and both LayerNorm tiles):
# median 1.3e-4, worst 5.4e-4 (draw 7 at 3,000 tokens, 2.3e-4 with the MLP weights compensated too), everything else <= 2.9e-4.
RAW_FP16C_BOUND = 6e-4


@pytest.mark.parametrize("wseed", range(8))
def test_fp16c_gate_over_weight_draws_and_lengths(built_lib, wseed):
    """The gate must not hinge on one weight draw or one length: the margin study of round 2 (tests/fp16c_margin.py,
    profiles/r02_fp16c_margin.txt) as a test -- eight seeded state dicts x {2,048, 3,000, 4,097, 8,193} tokens, batches of 4 random
    ACGT reads, one of them left-padded by a third.
    What is asserted: the RAW mode (MLP weights plain fp16, the guard's first level) is within RAW_FP16C_BOUND = 6e-4 on every
    batch -- UNDER the gate, where rounds 2-3 sat at it -- and the PRODUCT, `HyenaDna(precision="fp16c")` with its self-check on the
    loaded weights and on the batch (second level: MLP weights hi + lo too; then the exact-fp32 kernels), is within 5e-4 of the
    oracle wherever it kept a 16-bit form, and at the gate everywhere.  Round 4: 0 of 32 fall-backs (13 in round 3), one batch at
    the second level."""
    from chimeralm_amd import lm
    from chimeralm_amd.engine import Engine

    sdw = ho.make_state_dict(wseed, head_scale=3.0)
    e = Engine("cuda:0", precision="fp16c", chunk_reads=4)
    e.load_state_dict(sdw)
    ex = Engine("cuda:0", precision="fp16x3", chunk_reads=4)           # round 4: the same 32 batches through fp16x3 (bound: a tenth of the gate)
    ex.load_state_dict(sdw)
    worst = 0.0
    for L in (2048, 3000, 4097, 8193):
        rng = np.random.default_rng(1000 * wseed + L)
        ids = rng.integers(7, 11, size=(4, L)).astype(np.uint8)
        ids[:, -1] = 1
        ids[0, : L // 3] = 4
        ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sdw).numpy()
        t = torch.from_numpy(ids).cuda()
        got = e.forward(t).cpu().numpy()
        err = float(np.abs(got - ref).max())
        sc, _ = e.selfcheck(t)
        # the product path, a fresh module per length so that THIS batch is the one its self-check sees
        m = lm.ChimeraLM.new(precision="fp16c", chunk_reads=4)
        m.load_state_dict(sdw, strict=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = m.net(t).cpu().numpy()
        rep = m.net.selfcheck_report
        perr = float(np.abs(out - ref).max())
        print(f"weights {wseed}  L {L:5d}: raw |fp16c - oracle| {err:.2e}  (clm_selfcheck {sc:.2e})   guarded module: "
              f"{'FELL BACK to fp16x3' if rep['fallback'] else 'kept, MLP hi + lo' if rep.get('mlp_compensation') else 'kept'}"
              f" -> |logits - oracle| {perr:.2e}")
        errx = float(np.abs(ex.forward(t).cpu().numpy() - ref).max())
        print(f"      fp16x3 on the same batch: |fp16x3 - oracle| {errx:.2e}")
        assert errx <= TOL["fp16x3"]
        assert np.isfinite(got).all() and err <= RAW_FP16C_BOUND
        assert (got.argmax(1) == ref.argmax(1))[np.abs(ref[:, 0] - ref[:, 1]) > 2 * RAW_FP16C_BOUND].all()
        # the self-check referee (exact-fp32 kernels) is itself within ~2e-5 of the oracle: what it measures IS the mode's error
        assert abs(sc - err) <= 6e-5
        assert perr <= GATE and (out.argmax(1) == ref.argmax(1))[np.abs(ref[:, 0] - ref[:, 1]) > 2 * GATE].all()
        ran16 = not rep["fallback"] and m.net.engine(t.device).effective_precision(L) == "fp16c"
        print(f"      length switch measured on these weights: {rep.get('f16c_min_len')} tokens; this batch ran in {'fp16c' if ran16 else 'fp16x3'}")
        if ran16:
            assert perr <= 5e-4 + 6e-5                       # kept: this batch was measured within the threshold
        worst = max(worst, err)
        del m
    if wseed in (1, 2, 3):
        _check(e, "fp16c", _ids(6, 100, seed=60 + wseed), sdw)        # 100 tokens: the fp16x3 kernels inside the mode
    e.close(), ex.close()


def test_second_level_of_fp16c_is_closer_where_the_mlp_weights_show(built_lib):
    """clm_set_mlp_compensation: fc1 / fc2 on hi + lo weights.  On the study's MLP-sensitive weight draw (7) the first level's worst
    batch (3,000 tokens: 5.4e-4) drops to 2-3e-4; switching back restores the first level's logits bit for bit."""
    from chimeralm_amd.engine import Engine

    sdw = ho.make_state_dict(7, head_scale=3.0)
    rng = np.random.default_rng(1000 * 7 + 3000)
    ids = rng.integers(7, 11, size=(4, 3000)).astype(np.uint8)
    ids[:, -1] = 1
    ids[0, :1000] = 4
    ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sdw).numpy()
    e = Engine("cuda:0", precision="fp16c", chunk_reads=4)
    e.load_state_dict(sdw)
    t = torch.from_numpy(ids).cuda()
    l1 = e.forward(t).cpu().numpy()
    e.set_mlp_compensation(True)
    l2 = e.forward(t).cpu().numpy()
    e.set_mlp_compensation(False)
    assert np.array_equal(e.forward(t).cpu().numpy(), l1)
    e1, e2 = float(np.abs(l1 - ref).max()), float(np.abs(l2 - ref).max())
    print(f"weights 7, 4 x 3000: level 1 {e1:.2e}, level 2 {e2:.2e}")
    assert e2 < 0.7 * e1 and e2 <= 3.5e-4 and e1 <= RAW_FP16C_BOUND
    e32 = Engine("cuda:0", precision="fp32", chunk_reads=4)
    with pytest.raises(Exception, match="not a CLM_PREC_F16C handle"):
        e32.set_mlp_compensation(True)
    e.close(), e32.close()


def test_selfcheck_and_fallback_through_the_c_abi(engines, sd):
    """clm_selfcheck runs a batch through the handle's 16-bit mode AND the exact-fp32 kernels of the same handle:
    the difference it reports is exactly max |mode logits - fp32-engine logits|.  clm_set_fallback is a LEVEL (ABI 5): 1 makes every
    later forward of the 16-bit handle bit-identical to an fp16x3 engine's (the next arithmetic inside the gate: same kernels, same
    packing), 2 to the fp32 engine's, 0 undoes it; on an fp16x3 handle level 1 is exact fp32 (it did nothing there)."""
    from chimeralm_amd.engine import Engine, EngineError

    e, e32 = engines["fp16c"], engines["fp32"]
    ex = Engine("cuda:0", precision="fp16x3", chunk_reads=4)
    ex.load_state_dict(sd)
    for B, L in ((4, 2500), (3, 8193), (2, 16385)):
        t = torch.from_numpy(_ids(B, L, seed=301, pads=3)).cuda()
        a, r = e.forward(t).cpu(), e32.forward(t).cpu()
        diff, differ = e.selfcheck(t)
        assert diff == float((a - r).abs().max()) and 0 < diff <= GATE
        assert differ == int((a.argmax(1) != r.argmax(1)).sum())
        assert torch.equal(e.forward(t).cpu(), a)                          # the self-check leaves the mode as it was
        x = ex.forward(t).cpu()
        assert 0 < float((x - r).abs().max()) <= TOL["fp16x3"]
        e.set_fallback(1)
        assert e.effective_precision(L) == "fp16x3"
        assert torch.equal(e.forward(t).cpu(), x)
        assert e.selfcheck(t)[0] == diff                                   # not affected by the fallback level
        e.set_fallback(2)
        assert e.effective_precision(L) == "fp32"
        assert torch.equal(e.forward(t).cpu(), r)
        e.set_fallback(0)
        assert e.effective_precision(L) == "fp16c"
        assert torch.equal(e.forward(t).cpu(), a)
        if L == 2500:                                                      # an fp16x3 handle: level 1 = its own exact kernels
            ex.set_fallback(1)
            assert ex.effective_precision(L) == "fp32" and torch.equal(ex.forward(t).cpu(), r)
            assert ex.selfcheck(t)[0] == float((x - r).abs().max())        # (the mode on trial, whatever the level)
            ex.set_fallback(0)
            assert ex.effective_precision(L) == "fp16x3" and torch.equal(ex.forward(t).cpu(), x)
    with pytest.raises(EngineError, match="level must be"):
        e.set_fallback(3)
    short = torch.from_numpy(_ids(3, 700, seed=302)).cuda()                # the mode itself runs these in its fp16x3 kernels
    d_short, differ_short = e.selfcheck(short)
    assert e.effective_precision(700) == "fp16x3" and 0 < d_short <= TOL["fp16x3"] and differ_short == 0
    assert torch.equal(e.forward(short).cpu(), ex.forward(short).cpu())
    e.set_fallback(2)
    assert e.effective_precision(700) == "fp32" and torch.equal(e.forward(short).cpu(), e32.forward(short).cpu())
    e.set_fallback(0)
    assert e32.selfcheck(short) == (0.0, 0)
    e32.set_fallback(1)                                                    # an exact handle has nothing to fall back to
    assert e32.effective_precision(700) == "fp32"
    e32.set_fallback(0)
    ex.close()
    bf = engines["bf16"]                                                   # any 16-bit handle holds the referee
    d16, _ = bf.selfcheck(torch.from_numpy(_ids(3, 1000, seed=303)).cuda())
    assert GATE < d16 < TOL["bf16"]


def test_module_selfcheck_falls_back_to_fp16x3_when_the_mode_breaks(built_lib):
    """`HyenaDna(precision="fp16c")` measures the mode on the LOADED weights before its first batch (seeded synthetic reads at
    2,048 / 4,097 tokens + rows of the batch) and falls back above 5e-4 -- round 5: to fp16x3, the next-fastest arithmetic inside
    the gate, not to exact fp32.  Two weight sets: the seeded draw 0 with the head weights scaled x1 (the mode passes and stays)
    and x6 (seven head layers: logits and their errors grow ~20x over the parity tests' x3: the mode breaks; the module must
    notice, warn, and from then on give an fp16x3 engine's logits bit for bit -- which are within 1e-4 of the oracle)."""
    import warnings

    from chimeralm_amd import lm
    from chimeralm_amd.engine import Engine

    ids = torch.from_numpy(_ids(5, 3000, seed=311, pads=2).astype(np.int64)).cuda()
    good = ho.make_state_dict(0, head_scale=1.0)
    m = lm.ChimeraLM.new(precision="fp16c")
    m.load_state_dict(good, strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = m.net(ids)
    rep = m.net.selfcheck_report
    n_samples = len(rep["samples"])
    assert rep["fallback"] is False and 0 < rep["max_abs_dlogit"] <= 5e-4 and 3 <= n_samples <= 6
    assert rep["samples"][0]["sample"].startswith("synthetic 4 x 4097") and rep["samples"][-1]["sample"].startswith("batch rows")
    assert rep["f16c_min_len"] in (256, 512, 1024, 2048)                    # the length switch, measured on these weights
    ref = ho.forward(ids.cpu(), good)
    assert (out.cpu() - ref).abs().max() <= GATE
    eng = m.net.engine(ids.device)
    assert eng.effective_precision(3000) == "fp16c" and eng.effective_precision(rep["f16c_min_len"] - 1) == "fp16x3"
    m.net(ids)
    assert len(m.net.selfcheck_report["samples"]) == n_samples              # not again for a length inside the checked range ...
    short = ids[:, : rep["f16c_min_len"] + 40].contiguous()                 # ... but for a batch more than 1.5x shorter
    out_s = m.net(short)
    assert len(m.net.selfcheck_report["samples"]) == n_samples + (1 if 3 * short.shape[1] < 2 * 3000 else 0)
    assert (out_s.cpu() - ho.forward(short.cpu(), good)).abs().max() <= GATE

    bad = ho.make_state_dict(0, head_scale=6.0)
    m.load_state_dict(bad, strict=True)                                     # same module: new weights, new hearing
    e32 = Engine("cuda:0", precision="fp16x3", chunk_reads=64)
    e32.load_state_dict(bad)
    raw = Engine("cuda:0", precision="fp16c", chunk_reads=64)                # what the unguarded mode would answer
    raw.load_state_dict(bad)
    # (1) the longest sample (4,097 tokens) fails: the length switch goes above it, and this 3,000-token batch runs in the fp16x3
    #     kernels INSIDE the mode -- an fp16x3 engine's logits bit for bit, no fallback yet
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = m.net(ids)
    rep = m.net.selfcheck_report
    assert rep["fallback"] is False and rep["f16c_min_len"] == 4098 and m.net.engine(ids.device).effective_precision(3000) == "fp16x3"
    assert torch.equal(out.cpu(), e32.forward(ids).cpu())
    ref_bad = ho.forward(ids.cpu(), bad)
    assert (out.cpu() - ref_bad).abs().max() <= 5e-5 * ref_bad.abs().max()                # (logits up to +-60: 2e-5 relative measured)
    assert (raw.forward(ids).cpu() - out.cpu()).abs().max() > 5e-4
    # (2) a batch above the switch is judged by its own rows: both levels of the mode fail on it -> fp16x3 for good
    long_ids = torch.from_numpy(_ids(4, 6000, seed=312, pads=2).astype(np.int64)).cuda()
    with pytest.warns(RuntimeWarning, match="falling back to fp16x3"):
        out = m.net(long_ids)
    rep = m.net.selfcheck_report
    assert rep["fallback"] is True and rep["fallback_precision"] == "fp16x3" and rep["mlp_compensation"] is True and rep["max_abs_dlogit"] > 5e-4
    assert torch.equal(out.cpu(), e32.forward(long_ids).cpu())
    assert (raw.forward(long_ids).cpu() - out.cpu()).abs().max() > 5e-4
    e32.close(), raw.close()
    m2 = lm.ChimeraLM.new(precision="fp16c", selfcheck=False)               # opt-out: the raw mode
    m2.load_state_dict(bad, strict=True)
    assert m2.net(ids).shape == (5, 2) and m2.net.selfcheck_report == {}


def test_intermediates_fp32(engines, sd):
    B, L = 3, 257
    ids = _ids(B, L, pads=4)
    trace = {}
    ho.forward(torch.from_numpy(ids.astype(np.int64)), sd, trace=trace)
    e = engines["fp32"]
    e.forward(torch.from_numpy(ids).cuda())
    torch.cuda.synchronize()
    for name, shape, ref in (("hidden", (B, L, 256), trace["l3.out"]), ("scores", (B, L), trace["scores"]),
                             ("pooled", (B, 256), trace["pooled"])):
        got = e.debug_fetch(name, shape)
        scale = float(ref.abs().max())
        assert np.abs(got - ref.numpy()).max() <= 2e-5 * scale + 1e-6, name
    for i in range(4):
        k = e.debug_fetch(f"filter.{i}", (L, 256))
        assert np.abs(k - trace[f"l{i}.filter"].T.numpy()).max() <= 5e-5


def test_ids_dtypes_and_strides(engines, sd):
    ids = _ids(4, 200)
    e = engines["fp32"]
    a = e.forward(torch.from_numpy(ids).to(torch.int64).cuda()).cpu()
    b = e.forward(torch.from_numpy(ids).to(torch.int32).cuda()).cpu()
    c = e.forward(torch.from_numpy(ids).cuda()).cpu()                                   # uint8
    wide = torch.zeros(4, 333, dtype=torch.uint8).cuda()
    wide[:, :200] = torch.from_numpy(ids).cuda()
    d = e.forward(wide[:, :200]).cpu()                                                   # row stride 333
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_determinism_and_chunk_invariance(sd, built_lib):
    from chimeralm_amd.engine import Engine

    ids = torch.from_numpy(_ids(6, 700)).cuda()
    e1 = Engine("cuda:0", precision="fp16", chunk_reads=32)
    e2 = Engine("cuda:0", precision="fp16", chunk_reads=2)
    e1.load_state_dict(sd), e2.load_state_dict(sd)
    a, b, c = e1.forward(ids).cpu(), e1.forward(ids).cpu(), e2.forward(ids).cpu()
    assert torch.equal(a, b)                    # bit-identical run to run (no atomics, fixed reduction orders)
    assert torch.equal(a, c)                    # same read pairs in both chunkings -> identical bits
    solo = e1.forward(ids[1:2]).cpu()           # a read alone vs inside a batch (different pair partner)
    assert (solo - a[1:2]).abs().max() < 2e-3
    e1.close(), e2.close()


def test_token_capped_chunks_equal_small_chunks(sd, built_lib):
    """The engine lowers `chunk_reads` for long reads so that a chunk holds at most 256 x 8,256 tokens (clm_api.hip, chunk_for):
    110 reads of 20,000 tokens go through as chunks of 104 + 6 reads under the default of 256 and agree with chunks of 8 (the same
    read pairs in the packed transform; not bitwise: where a workgroup's tile range starts inside a read, its first two tokens take
    the gated hand-over's patch path, and the ranges follow the launch size); the workspace follows the capped chunk, not 256 reads."""
    from chimeralm_amd.engine import Engine

    ids = torch.from_numpy(_ids(110, 20000, seed=5)).cuda()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    e1 = Engine("cuda:0", precision="fp16c")                  # default chunk_reads = 256
    e1.load_state_dict(sd)
    a = e1.forward(ids).cpu()
    used = free0 - torch.cuda.mem_get_info()[0]
    assert torch.isfinite(a).all()
    # z + y + h + gscratch of 104 reads x 20,032 tokens: ~12 GB; 256 reads would be ~30 GB
    assert used < 16 * 2 ** 30, f"workspace of {used / 2 ** 30:.1f} GiB: the chunk was not capped"
    e2 = Engine("cuda:0", precision="fp16c", chunk_reads=8)
    e2.load_state_dict(sd)
    assert (a - e2.forward(ids).cpu()).abs().max() < 0.5 * GATE
    e1.close(), e2.close()


@pytest.mark.parametrize("L", [9000, 16385])
def test_block0_id_table_long_reads(sd, built_lib, monkeypatch, L):
    """Same for the segmented kernel (L > 8193), incl. the dot-product path of the lone last token (16385)."""
    from chimeralm_amd.engine import Engine

    ids = _ids(3, L, seed=6, pads=3).astype(np.int64)
    ids[0, 8190:8196] = [11, 0, 1, 2, 3, 15]                # specials across the first segment boundary
    t = torch.from_numpy(ids).cuda()
    e1 = Engine("cuda:0", precision="fp16", chunk_reads=4)
    monkeypatch.setenv("CLM_DEBUG", "no_idconv")
    e2 = Engine("cuda:0", precision="fp16", chunk_reads=4)
    monkeypatch.delenv("CLM_DEBUG")
    e1.load_state_dict(sd), e2.load_state_dict(sd)
    a, b = e1.forward(t).cpu(), e2.forward(t).cpu()
    assert (a - b).abs().max() < TOL["fp16"]
    e1.close(), e2.close()


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_block0_id_table_convolution_matches_in_proj_path(sd, built_lib, monkeypatch, prec):
    """16-bit modes skip block 0's in_proj: the convolution looks x0|x1|v up by token id (ztab).  Same logits as the
    explicit in_proj path (CLM_DEBUG=no_idconv) up to the 16-bit rounding of z that the table path does not have; covers every
    row of the 16-row embedding table (specials, N, the padding rows 12-15) and both read parities of a pair."""
    from chimeralm_amd.engine import Engine

    ids = _ids(5, 1000, seed=5).astype(np.int64)
    ids[0, :16] = np.arange(16)
    ids[1, -3:] = [12, 13, 15]                  # rows of the 16-row table beyond the 12-token vocabulary
    t = torch.from_numpy(ids).cuda()
    e1 = Engine("cuda:0", precision=prec, chunk_reads=8)
    monkeypatch.setenv("CLM_DEBUG", "no_idconv")
    e2 = Engine("cuda:0", precision=prec, chunk_reads=8)
    monkeypatch.delenv("CLM_DEBUG")
    e1.load_state_dict(sd), e2.load_state_dict(sd)
    a, b = e1.forward(t).cpu(), e2.forward(t).cpu()
    assert (a - b).abs().max() < TOL[prec]
    decided = (b[:, 0] - b[:, 1]).abs() > MARGIN[prec]
    assert torch.equal(a.argmax(1)[decided], b.argmax(1)[decided])
    e1.close(), e2.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16c", "fp16"])
def test_full_size_8k_reads(engines, sd, prec):
    """BASELINE config size (8192 bases + [SEP] = 8193 tokens, FFT size 16384 with the aliased tail)."""
    ids = _ids(3, 8193, seed=11)
    _check(engines[prec], prec, ids, sd)


@pytest.mark.parametrize("prec,B,L", [("fp16", 3, 129), ("fp16", 4, 385), ("bf16", 2, 1025), ("fp16c", 3, 2049), ("fp16c", 5, 8193),
                                      ("fp16c", 2, 16385)])
def test_lone_last_token_is_peeled_off_the_tile_kernels(sd, built_lib, monkeypatch, prec, B, L):
    """Reads of 128 k + 1 tokens: the last token (the [SEP] of every 8k-bp read) is causally isolated in the backbone and runs
    through fp32 matrix-vector kernels instead of a 128-token tile of its own (csrc/lone_token.hip).  Same logits as with the
    token kept in the tile kernels (CLM_DEBUG=no_lone_peel) up to that one token's 16-bit roundings, both within the mode's bound
    of the oracle; read 0 of the batch is all [PAD] but for its [SEP] (left padding to the extreme)."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=83, pads=3)
    ids[0, : L - 1] = 4                                         # read 0: pads only, then [SEP]
    t = torch.from_numpy(ids).cuda()
    e0 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.setenv("CLM_DEBUG", "no_lone_peel")
    e1 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.delenv("CLM_DEBUG")
    e0.load_state_dict(sd), e1.load_state_dict(sd)
    a, b = e0.forward(t).cpu(), e1.forward(t).cpu()
    assert torch.equal(a, e0.forward(t).cpu())                  # deterministic
    assert (a - b).abs().max() < TOL[prec]
    _check(e0, prec, ids, sd)
    e0.close(), e1.close()


@pytest.mark.parametrize("prec,B,L,env", [("fp16c", 5, 8193, "conv_oneshot"), ("fp16c", 3, 6000, "conv_oneshot"),
                                          ("bf16", 4, 4098, "conv_oneshot"), ("fp16c", 5, 8193, "conv_no_xcd"),
                                          ("fp16c", 3, 20000, "conv_no_xcd")])
def test_persistent_convolution_equals_one_workgroup_per_unit(sd, built_lib, monkeypatch, prec, B, L, env):
    """Reads of 4,098..8,193 tokens in the 16-bit modes run through hyena_conv_pers_kernel (persistent workgroups, next unit's rows
    requested behind the last inverse pass, XCD-aware unit order; block 0: its id-table variant).  Against hyena_conv_kernel
    (CLM_DEBUG=conv_oneshot) the same transform but x0's short filter evaluated in phase C: fp32-rounding-level differences in y that
    flip a few 16-bit roundings -- logits agree to a fraction of the mode's error, and both kernels stand against the oracle.
    The plain unit order (CLM_DEBUG=conv_no_xcd) only permutes which workgroup does which unit: bit-identical, for the segmented
    long-read kernel too (20,000 tokens).  Odd batches: a unit with one read."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=97, pads=3)
    t = torch.from_numpy(ids).cuda()
    e0 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.setenv("CLM_DEBUG", env)                 # read by clm_create
    e1 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.delenv("CLM_DEBUG")
    e0.load_state_dict(sd), e1.load_state_dict(sd)
    a, b = e0.forward(t).cpu(), e1.forward(t).cpu()
    if env == "conv_no_xcd":
        assert torch.equal(a, b), (a - b).abs().max().item()
    else:
        assert (a - b).abs().max() < 0.3 * TOL[prec]          # a fraction of the mode's own error bound
        _check(e1, prec, ids, sd)
    e0.close(), e1.close()


@pytest.mark.parametrize("prec,B,L", [("fp32", 5, 8193), ("fp32", 3, 6000), ("fp16x3", 4, 4098)])
def test_persistent_convolution_of_the_exact_engine(sd, built_lib, monkeypatch, prec, B, L):
    """Round 5: the exact / fp16x3 engine's fp32 rows (raw x0 | x1 | v; block 0 by token id) go through hyena_conv_pers_kernel as
    well.  Same transform as hyena_conv_kernel (CLM_DEBUG=conv_oneshot) with x0's short filter evaluated after it: logits agree at
    fp32-rounding level, and the persistent form stands against the oracle by itself.  Odd batch: a unit with one read."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=98, pads=3)
    t = torch.from_numpy(ids).cuda()
    e0 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.setenv("CLM_DEBUG", "conv_oneshot")      # read by clm_create
    e1 = Engine("cuda:0", precision=prec, chunk_reads=4)
    monkeypatch.delenv("CLM_DEBUG")
    e0.load_state_dict(sd), e1.load_state_dict(sd)
    a, b = e0.forward(t).cpu(), e1.forward(t).cpu()
    assert torch.equal(a, e0.forward(t).cpu())           # deterministic
    assert (a - b).abs().max() < 2e-5, (a - b).abs().max().item()
    _check(e0, prec, ids, sd)
    e0.close(), e1.close()


@pytest.mark.parametrize("B,L", [(3, 257), (5, 64), (2, 65), (1, 1), (4, 1000), (3, 8193), (2, 20000), (7, 130)])
def test_fused_fp32_tail_equals_the_separate_gemm_kernels(sd, built_lib, monkeypatch, B, L):
    """Exact fp32 runs one fused kernel per block tail since round 4 (tail32.hip: out_proj + LN2 + MLP + both residuals + the next
    block's LN1 / in_proj on 64-token tiles).  Against the five separate GEMM kernels of rounds 1-3 (CLM_DEBUG=unfused_fp32) the same
    fp32 products in another summation order: logits agree to fp32 rounding, and both stand against the oracle at the exact mode's
    bound.  Tiles that end inside a read, reads shorter than a tile, one token, pads, the segmented long-read path."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=61, pads=2 if L > 8 else 0)
    t = torch.from_numpy(ids).cuda()
    e0 = Engine("cuda:0", precision="fp32")
    monkeypatch.setenv("CLM_DEBUG", "unfused_fp32")      # read by clm_create
    e1 = Engine("cuda:0", precision="fp32")
    monkeypatch.delenv("CLM_DEBUG")
    e0.load_state_dict(sd), e1.load_state_dict(sd)
    a, b = e0.forward(t).cpu(), e1.forward(t).cpu()
    h0 = e0.debug_fetch("h", (B, L, 256)).copy()
    h1 = e1.debug_fetch("h", (B, L, 256)).copy()
    scale = float(np.abs(h1).max())
    print(f"fp32 fused vs separate kernels, {B} x {L}: |dlogit| {(a - b).abs().max().item():.2e}, stream {np.abs(h0 - h1).max():.2e} of {scale:.3g}")
    assert (a - b).abs().max() <= 2e-5
    assert np.abs(h0 - h1).max() <= 1e-5 * scale
    _check(e0, "fp32", ids, sd)
    e0.close(), e1.close()


@pytest.mark.parametrize("prec,B,L", [("fp16c", 5, 8193), ("fp16c", 3, 6000), ("fp16c", 4, 4097), ("fp16", 3, 1000), ("bf16", 2, 300),
                                      ("fp16c", 3, 20000), ("fp16c", 2, 16385), ("fp16", 7, 2049), ("fp16c", 1, 8193)])
def test_gated_hand_over_equals_raw_rows(sd, built_lib, monkeypatch, prec, B, L):
    """Round 3: the fused tail kernel's in_proj stage applies the next block's short filter and the x1 * v gate itself and hands
    the convolution x0f and g (two rows per channel instead of x0 | x1 | v); tiles go to the workgroups in contiguous ranges, the
    filter's two-token history travels from tile to tile in LDS, the first two tokens of a range that starts inside a read are
    recomputed by a patch kernel, the peeled last token takes its history from the read's last tile.  Against the previous
    hand-over (CLM_DEBUG=raw_z: three rows, filtered and gated by the convolution): the same arithmetic up to WHERE the 16-bit
    rounding of z sits (before the filter then, after it now) -- logits agree to a fraction of the mode's bound, and both stand
    against the oracle.  Shapes: persistent 8k kernel (full and ragged units, odd batch, a lone read), one-shot kernels of three
    transform sizes, the segmented kernel with and without its dot-product tail; 5 x 64 tiles on 256 workgroups = ranges of 2
    tiles (a patched boundary every second tile), 1 x 64 tiles = one tile per workgroup (every tile patched)."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=131, pads=3)
    t = torch.from_numpy(ids).cuda()
    e0 = Engine("cuda:0", precision=prec, chunk_reads=8)
    monkeypatch.setenv("CLM_DEBUG", "raw_z")
    e1 = Engine("cuda:0", precision=prec, chunk_reads=8)
    monkeypatch.delenv("CLM_DEBUG")
    e0.load_state_dict(sd), e1.load_state_dict(sd)
    a, b = e0.forward(t).cpu(), e1.forward(t).cpu()
    assert torch.equal(a, e0.forward(t).cpu())                  # deterministic
    assert (a - b).abs().max() < 0.4 * TOL[prec]
    ea = _check(e0, prec, ids, sd)
    eb = _check(e1, prec, ids, sd)
    print(f"{prec} {B} x {L}: |gated - oracle| {ea:.2e}  |raw rows - oracle| {eb:.2e}  |gated - raw| {(a - b).abs().max():.2e}")
    e0.close(), e1.close()


@pytest.mark.parametrize("prec,B,L", [("fp32", 3, 8194), ("fp32", 2, 16385), ("fp16", 3, 20000), ("fp16", 3, 24577),
                                      ("fp32", 1, 8200), ("fp16c", 3, 20000), ("fp16c", 2, 16385)])
def test_long_reads_segmented_convolution(engines, sd, prec, B, L):
    """L > 8193: partitioned convolution over 8192-token segments (2 and 3 segments, odd batch, a last segment of 1, 2 and 8 tokens;
    lengths S*8192 + 1 take the dot-product path for the lone last token: 16385 in fp32, 24577 in fp16 with an odd batch)."""
    _check(engines[prec], prec, _ids(B, L, seed=21, pads=5), sd)


def test_maximum_length_reads(engines, sd):
    """The longest input the reference can produce: tokenizer.max_len_single_sentence = 32769 tokens (bam.py:155-166), i.e.
    5 convolution segments, the last one holding a single token."""
    ids = _ids(2, 32769, seed=31)
    ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sd).numpy()
    _check(engines["fp16c"], "fp16c", ids, sd, ref=ref)
    _check(engines["fp16"], "fp16", ids, sd, ref=ref)


@pytest.mark.parametrize("prec,B,chunk,L", [("fp16c", 256, 256, 8193), ("fp16c", 256, 64, 8193), ("fp16c", 32, 256, 8193),
                                            ("fp16", 256, 64, 8193), ("fp16c", 4, 256, 32769), ("fp16c", 32, 256, 32769)])
def test_baseline_batch_size_independent_properties(sd, built_lib, prec, B, chunk, L):
    """BASELINE.json's bench configurations AT SIZE and in the benched mode: 256 reads of 8192 bases + [SEP] as ONE chunk (the
    default since round 3: 32,768 convolution units per launch through the persistent XCD-ordered loop, 16,384 tail tiles, z alone
    3.2 GB) and in 64-read chunks (C3 as benched in round 2), and the 32-read shard a GPU gets in the 8-GPU run (C4).  The oracle is too slow for the whole batch; reads are independent units, so (a) two runs
    are bit-identical, (b) reversing the batch reverses the logits (each read gets another pair partner in the packed FFT:
    equal up to rounding, not bitwise), (c) reads computed alone equal their rows of the full batch, (d) a sample of rows
    matches the oracle at the mode's bound (fp16c: GATE), (e) fp16c: the exact-fp32 kernels agree on a sample (clm_selfcheck).
    Round 4 (VERDICT r03 missing #6): C5 at ITS sizes too -- 32 reads of 32,768 bases + [SEP] (segmented convolution with the
    dot-product tail, token-capped chunks of 64 reads) and the 4-read shard a GPU gets in the 8-GPU run; two oracle rows there."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=41)
    t = torch.from_numpy(ids).cuda()
    e = Engine("cuda:0", precision=prec, chunk_reads=chunk)
    e.load_state_dict(sd)
    a = e.forward(t).cpu()
    assert torch.isfinite(a).all()
    assert torch.equal(a, e.forward(t).cpu())                                   # (a)
    r = e.forward(torch.flip(t, dims=[0]).contiguous()).cpu()
    assert (torch.flip(r, dims=[0]) - a).abs().max() < 0.5 * TOL[prec]           # (b)
    pick = sorted({0, max(B // 4 - 1, 0), B // 4, B - max(B // 5, 1), B - 1})
    solo = e.forward(t[pick].contiguous()).cpu()
    assert (solo - a[pick]).abs().max() < 0.5 * TOL[prec]                        # (c)
    small = Engine("cuda:0", precision=prec, chunk_reads=4)                      # ... and EVERY row against 4-read chunks
    small.load_state_dict(sd)
    d_small = (small.forward(t).cpu() - a).abs().max().item()
    small.close()
    print(f"{prec} {B} x {L} (chunk {chunk}): every row against 4-read chunks {d_small:.2e}")
    assert d_small < 0.5 * TOL[prec]
    n_ref = 3 if L <= 8193 else 2                                                # (the oracle takes ~10 s per 32k-token read)
    ref = ho.forward(torch.from_numpy(ids[pick[:n_ref]].astype(np.int64)), sd)   # (d)
    err = (a[pick[:n_ref]] - ref).abs().max()
    print(f"{prec} {B} x {L} (chunk {chunk}): |logits - oracle| on rows {pick[:n_ref]} = {err:.2e}")
    assert err <= TOL[prec]
    decided = (ref[:, 0] - ref[:, 1]).abs() > MARGIN[prec]
    assert torch.equal(a[pick[:n_ref]].argmax(1)[decided], ref.argmax(1)[decided])
    if prec == "fp16c":                                                          # (e)
        diff, _ = e.selfcheck(t[max(B - 8, 0):].contiguous())
        assert 0 < diff <= GATE
    e.close()


_ORACLE_ROWS: dict = {}


def _oracle_rows(ids: np.ndarray, rows: list[int], sd: dict) -> torch.Tensor:
    """Oracle logits of ids[rows], one read at a time, kept per (weights, read) for the other cases of the module that hold that read."""
    out = []
    for r in rows:
        key = (id(sd), ids[r].tobytes())
        if key not in _ORACLE_ROWS:
            _ORACLE_ROWS[key] = ho.forward(torch.from_numpy(ids[r: r + 1].astype(np.int64)), sd)[0]
        out.append(_ORACLE_ROWS[key])
    return torch.stack(out)


def _bench_ids(B: int, L: int) -> tuple[np.ndarray, list[int]]:
    """The reads of the bench-shape cases and the rows held to the oracle.  8,193 tokens: 256 reads whose last quarter (192-255) is
    left-padded with [PAD] runs of varied length, as the collator pads shorter reads; the 32-read case is rows 0-23 and 248-255 of
    it.  32,769 tokens: 32 reads; the 4-read case is rows 0-2 and 31.  The oracle rows (first, a padded row at index >= 128 or in the
    last quarter, last) are the same reads in every case of one length."""
    if L == 8193:
        ids = _ids(256, L, seed=43)
        rng = np.random.default_rng(8193)
        for r in range(192, 256):
            ids[r, : int(rng.integers(1, L - 64))] = 4
        if B == 256:
            return ids, [0, 250, 255]
        return ids[list(range(24)) + list(range(248, 256))], [0, 26, 31]
    ids = _ids(32, L, seed=47)
    return (ids, [0, 31]) if B == 32 else (ids[[0, 1, 2, 31]], [0, 3])


@pytest.mark.parametrize("prec,B,chunk,L", [("fp32", 256, 256, 8193), ("fp16x3", 256, 256, 8193), ("fp16x3", 32, 256, 8193),
                                            ("fp32", 32, 256, 32769), ("fp16x3", 32, 256, 32769), ("fp16x3", 4, 256, 32769)])
def test_exact_and_fp16x3_at_bench_shapes(sd, built_lib, prec, B, chunk, L):
    """The two arithmetics the product's safety rests on -- exact fp32 (the referee of every self-check) and fp16x3 (fp16c's short
    reads and first fall-back level) -- at the bench's shapes in one chunk: 256 x 8,193 is 32,768 persistent-convolution units and
    6.5 GB of fp32 z rows (byte offsets past 4 GB), 32 x 32,769 the segmented convolution.  (a) finite, bit-identical on a second
    run; (b) EVERY row equals a handle of 4-read (2 at 32,769) chunks up to the read pairing of the packed FFT; (c) oracle rows within
    1e-4, labels where the oracle decides them; (d) fp16x3: it runs fp16x3, an exact-fp32 handle agrees on every row, and its
    self-check on 8 rows spread over the batch passes."""
    from chimeralm_amd.engine import Engine

    ids, rows = _bench_ids(B, L)
    t = torch.from_numpy(ids).cuda()
    e = Engine("cuda:0", precision=prec, chunk_reads=chunk)
    e.load_state_dict(sd)
    a = e.forward(t).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, e.forward(t).cpu())       # (a)
    small = Engine("cuda:0", precision=prec, chunk_reads=4 if L <= 8193 else 2)
    small.load_state_dict(sd)
    d_small = (small.forward(t).cpu() - a).abs().max().item()                   # (b)
    small.close()
    ref = _oracle_rows(ids, rows, sd)                                            # (c)
    err = (a[rows] - ref).abs().max().item()
    msg = f"{prec} {B} x {L}: every row vs small chunks {d_small:.2e}, rows {rows} vs oracle {err:.2e}"
    if prec == "fp16x3":                                                         # (d)
        assert e.effective_precision(L) == "fp16x3"
        e32 = Engine("cuda:0", precision="fp32", chunk_reads=chunk)
        e32.load_state_dict(sd)
        d32 = (e32.forward(t).cpu() - a).abs().max().item()
        e32.close()
        sel = sorted({round(i * (B - 1) / 7) for i in range(8)})
        diff, flips = e.selfcheck(t[sel].contiguous())
        msg += f", every row vs exact fp32 {d32:.2e}, selfcheck on rows {sel} {diff:.2e}"
        assert d32 <= 1e-4 and 0 < diff <= 1e-4 and flips == 0, msg
    print(msg)
    assert d_small <= 2e-5, msg
    assert err <= 1e-4, msg
    decided = (ref[:, 0] - ref[:, 1]).abs() > MARGIN["fp16x3"]
    assert torch.equal(a[rows].argmax(1)[decided], ref.argmax(1)[decided])
    e.close()


def _big_weight_sd(value: float) -> dict:
    sdw = ho.make_state_dict(0, head_scale=3.0)
    sdw["net.backbone.backbone.layers.1.mixer.in_proj.weight"][5, 17] = value
    return sdw


@pytest.mark.parametrize("value", [300.0, 100.0, 63.9])
def test_fp16x3_weight_range_of_the_engine(built_lib, value):
    """fp16x3 packs weights x 2^10 as fp16 hi + lo: the hi half saturates from |w| ~ 63.97, the lo half absorbs the rest at reduced
    precision up to ~128, above that the weight is clamped.  A handle whose x3-packed weights reach 64 runs exact fp32 wherever it
    would run fp16x3 -- an fp16x3 handle, fp16c's short reads and its first fall-back level -- and says so; just below, it stays."""
    from chimeralm_amd.engine import Engine

    sdw = _big_weight_sd(value)
    ids = _ids(3, 1000, seed=61)
    ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sdw)
    t = torch.from_numpy(ids).cuda()
    want = "fp32" if value >= 64 else "fp16x3"
    ex = Engine("cuda:0", precision="fp16x3", chunk_reads=4)
    ex.load_state_dict(sdw)
    err = (ex.forward(t).cpu() - ref).abs().max().item()
    msg = [f"fp16x3 handle ({ex.effective_precision(1000)}) {err:.2e}"]
    assert ex.effective_precision(1000) == want, msg
    if value >= 64:
        fc = Engine("cuda:0", precision="fp16c", chunk_reads=4)
        fc.load_state_dict(sdw)
        for level in (0, 1):
            fc.set_fallback(level)
            err_c = (fc.forward(t).cpu() - ref).abs().max().item()
            msg.append(f"fp16c level {level} ({fc.effective_precision(1000)}) {err_c:.2e}")
            assert fc.effective_precision(1000) == "fp32", msg
            assert err_c <= 1e-4, msg
        fc.close()
    print(f"|w| = {value}: |logits - oracle| " + ", ".join(msg))
    assert err <= 1e-4, msg
    ex.close()


@pytest.mark.parametrize("prec", ["fp16x3", "fp16c"])
def test_fp16x3_weight_range_of_the_module(built_lib, caplog, prec):
    """`HyenaDna` reads the engine's arithmetic back at the weight load: a warning naming exact fp32 and a `precision_report` of what
    runs where the mode would use fp16x3; weights inside the range report no fall-back."""
    from chimeralm_amd import lm

    sdw = _big_weight_sd(300.0)
    ids = _ids(3, 1000, seed=61)
    ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sdw)
    model = lm.ChimeraLM.new(precision=prec, chunk_reads=4)
    model.load_state_dict(sdw, strict=True)
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got, _ = model.predict_step({"input_ids": torch.from_numpy(ids).cuda(), "labels": torch.full((3,), -1)}, 0)
    rep = model.net.precision_report
    assert rep["precision"] == prec and rep["fallback"] is True and rep["fallback_precision"] == "fp32" and rep["max_abs_weight"] == 300.0
    assert any("exact-fp32" in r.getMessage() and prec in r.getMessage() for r in caplog.records)
    if model.net.selfcheck_report.get("fallback"):
        assert model.net.selfcheck_report["fallback_precision"] == "fp32"
    err = (got.cpu() - ref).abs().max().item()
    print(f"HyenaDna {prec} with |w| = 300: |logits - oracle| {err:.2e}, report {rep}")
    assert err <= (1e-4 if prec == "fp16x3" else GATE)
    ok = lm.ChimeraLM.new(precision=prec, chunk_reads=4)
    ok.load_state_dict(ho.make_state_dict(0, head_scale=3.0), strict=True)
    ok.predict_step({"input_ids": torch.from_numpy(ids).cuda(), "labels": torch.full((3,), -1)}, 0)
    assert ok.net.precision_report["fallback"] is False and ok.net.precision_report["max_abs_weight"] < 64


@pytest.mark.parametrize("wseed,B,L,pads", [(0, 3, 257, 0), (0, 2, 64, 0), (0, 1, 1, 0), (4, 5, 130, 3), (4, 4, 1000, 0), (7, 3, 2049, 5),
                                            (7, 2, 8193, 0), (0, 2, 20000, 0)])
def test_fp16x3_is_fp32_class(built_lib, wseed, B, L, pads):
    """`fp16x3` (round 4, csrc/tail32.hip AR_X3): the exact engine's fused block tails with every operand of a product split into
    two halfs (hi = fp16(x), lo = fp16(x - hi)) and three fp16 MFMAs per product.  Held to a TENTH of the gate against the oracle
    and against the exact-fp32 engine on the same ids -- measured: as far from the fp64-checked oracle as exact fp32 itself is
    (~1e-5) -- over three weight draws, one-token to long reads, ragged tiles and pads."""
    from chimeralm_amd.engine import Engine

    sdw = ho.make_state_dict(wseed, head_scale=3.0)
    ids = _ids(B, L, seed=71 + L, pads=pads if L > 8 else 0)
    t = torch.from_numpy(ids).cuda()
    e32, ex = Engine("cuda:0", precision="fp32"), Engine("cuda:0", precision="fp16x3")
    e32.load_state_dict(sdw), ex.load_state_dict(sdw)
    assert ex.effective_precision(L) == "fp16x3"
    a, b = e32.forward(t).cpu(), ex.forward(t).cpu()
    assert torch.equal(b, ex.forward(t).cpu())                                   # deterministic
    d32 = (a - b).abs().max().item()
    diff, flips = ex.selfcheck(t)                                                # the handle's own referee pass: its exact-fp32 tails
    assert abs(diff - d32) <= 1e-6 and flips == 0
    msg = f"weights {wseed}, {B} x {L}: |fp16x3 - exact fp32| {d32:.2e}"
    assert d32 <= TOL["fp16x3"]
    if L <= 2049:
        err = _check(ex, "fp16x3", ids, sdw)
        msg += f", |fp16x3 - oracle| {err:.2e}"
    print(msg)
    e32.close(), ex.close()


@pytest.mark.parametrize("prec,B,L,cut", [("fp32", 3, 8193, 5000), ("fp16c", 6, 8193, 4097), ("fp16c", 2, 32769, 20000), ("fp16", 5, 3000, 1500)])
def test_the_residual_stream_is_causal(sd, built_lib, prec, B, L, cut):
    """A property of the operator that does not need the oracle, at the bench's read lengths: the backbone is causal (the long
    filter is applied as a causal convolution -- zero-padded to twice the length, hyena.py:244-256 through the backbone's fftconv --
    and everything else is token-wise), so bases after position `cut` cannot move the residual stream at or before it.  The FFT
    mixes every position of a read (and of its pair partner in the packed transform), so the claim holds to rounding, not
    bitwise: the stream before the cut must agree to a few parts in 1e5 of its scale, while the stream after it must move."""
    from chimeralm_amd.engine import Engine

    ids = _ids(B, L, seed=53)
    ids2 = ids.copy()
    ids2[:, cut:L - 1] = _ids(B, L, seed=54)[:, cut:L - 1]                       # (the closing [SEP] stays)
    assert (ids2[:, cut:] != ids[:, cut:]).mean() > 0.5
    e = Engine("cuda:0", precision=prec)
    e.load_state_dict(sd)
    e.forward(torch.from_numpy(ids).cuda())
    h1 = e.debug_fetch("h", (B, L, 256)).copy()
    e.forward(torch.from_numpy(ids2).cuda())
    h2 = e.debug_fetch("h", (B, L, 256)).copy()
    e.close()
    scale = float(np.abs(h1).max())
    before = float(np.abs(h1[:, :cut] - h2[:, :cut]).max())
    after = float(np.abs(h1[:, cut:L - 1] - h2[:, cut:L - 1]).max())
    print(f"{prec} {B} x {L}, cut {cut}: stream scale {scale:.3g}, moved before the cut {before:.2e}, after {after:.2e}")
    assert np.isfinite(h1).all() and np.isfinite(h2).all()
    # (fp16c: z / y travel at ~15 bits; plain fp16: at 11 -- an FFT-rounding-level change flips a half's last bit: 2^-11 of the element)
    assert before <= {"fp32": 2e-6, "fp16c": 1e-4, "fp16": 1e-3}[prec] * scale
    assert after > 1e-2 * scale


def test_shape_churn_filter_cache_and_workspace_regrowth(sd, built_lib):
    """A stream of batches of changing shape through ONE engine: the filter sets (one per transform size, one for long reads) are built on
    first use, the workspace grows on demand, short and long-read kernels alternate.  Every result must equal the one the
    same shape gave the first time (bit-identical: no state leaks between calls), and the short ones the oracle's."""
    from chimeralm_amd.engine import Engine

    e = Engine("cuda:0", precision="fp16", chunk_reads=4)
    e.load_state_dict(sd)
    rng = np.random.default_rng(17)
    shapes = [(2, 300), (5, 1000), (1, 9000), (3, 129), (2, 16385), (7, 2049), (1, 2), (4, 8193), (3, 8200)]
    first = {}
    order = list(range(len(shapes))) * 3
    rng.shuffle(order)
    for k in order:
        B, L = shapes[k]
        ids = _ids(B, L, seed=100 + k)
        out = e.forward(torch.from_numpy(ids).cuda()).cpu()
        assert torch.isfinite(out).all()
        if k not in first:
            first[k] = out
            if L <= 2049:
                ref = ho.forward(torch.from_numpy(ids.astype(np.int64)), sd)
                assert (out - ref).abs().max() <= TOL["fp16"]
        else:
            assert torch.equal(out, first[k]), f"shape {shapes[k]} changed after other shapes ran"
    e.close()


def test_random_shapes_against_the_exact_kernels(sd, built_lib):
    """Forty seeded (reads, tokens) shapes -- odd and even batches, lengths on and off the 64 / 128 / 8,192-token boundaries, padded
    reads -- through ONE default fp16c engine (256-read chunks, gated hand-over, peeled last token where L = 128 k + 1): every
    batch within the mode's regression bound of the exact-fp32 kernels of the same engine (`clm_selfcheck`) and label-identical
    where decided.  A cheap sweep for indexing mistakes the hand-picked shapes above might miss."""
    from chimeralm_amd.engine import Engine

    e = Engine("cuda:0", precision="fp16c")
    e.load_state_dict(sd)
    e.set_f16c_min_len(1)                                     # the 16-bit kernels at every length
    rng = np.random.default_rng(2026)
    special = [127, 128, 129, 255, 257, 1025, 2049, 4097, 8191, 8192, 8193, 8194, 8257, 9000, 16384, 16385, 16386, 24577]
    worst = 0.0
    for k in range(40):
        L = int(special[k]) if k < len(special) else int(rng.integers(2, 12000))
        B = int(rng.integers(1, 9)) if L > 6000 else int(rng.integers(1, 40))
        ids = _ids(B, L, seed=500 + k)
        if k % 3 == 0 and L > 40:
            ids[0, : L // 3] = 4                                # a left-padded read
        t = torch.from_numpy(ids).cuda()
        out = e.forward(t).cpu()
        assert torch.isfinite(out).all(), (B, L)
        diff, differ = e.selfcheck(t)
        worst = max(worst, diff)
        bound = RAW_FP16C_BOUND if L >= 1024 else 4e-3           # short reads: less to average over (section 2)
        assert diff <= bound, f"{B} x {L}: |fp16c - exact fp32| = {diff:.2e}"
    print(f"40 random shapes: worst |fp16c - exact fp32| = {worst:.2e}")
    e.close()


def test_collated_bam_batch_against_oracle(engines, sd, golden_dir):
    """configs[0] plumbing: real reads -> tokenizer -> collator (left pad) -> engine == oracle on the same batch."""
    from chimeralm_amd import bam, tokenizer as T

    tok = T.CharTokenizer(model_max_length=3000, padding_side="left")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=golden_dir / "test_chimric_reads.bam", batch_size=6,
                           max_predict_samples=12)
    dm.setup("predict")
    for batch in dm.predict_dataloader():
        ids = batch["input_ids"]
        assert ids.shape[1] <= 2999 and (ids == 4).any()                                 # ragged -> padded
        ref = ho.forward(ids, sd).numpy()
        got = engines["fp32"].forward(ids.cuda()).cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-3
        assert do.prediction_lines(got, batch["id"].numpy()) == do.prediction_lines(ref, batch["id"].numpy())


def test_module_boundary_and_writer(sd, tmp_path, built_lib):
    """The drop-in boundary: ClassificationLit(net=HyenaDna(...)).predict_step + PredictionWriter files."""
    from types import SimpleNamespace

    from chimeralm_amd import lm
    from chimeralm_amd.callbacks import PredictionWriter
    from chimeralm_amd.tokenizer import pack_read_name

    model = lm.ChimeraLM.new(precision="fp32")
    model.load_state_dict(sd, strict=True)
    ids_np = _ids(4, 150)
    batch = {"input_ids": torch.from_numpy(ids_np.astype(np.int64)).cuda(),
             "labels": torch.full((4,), -1), "id": torch.tensor([pack_read_name(f"r{i}") for i in range(4)]).to(torch.int8)}
    logits, labels = model.predict_step(batch, 0)
    ref = ho.forward(torch.from_numpy(ids_np.astype(np.int64)), sd)
    assert (logits.cpu() - ref).abs().max() < 1e-3 and (labels == -1).all()
    PredictionWriter(tmp_path, "batch").write_on_batch_end(SimpleNamespace(global_rank=0), model, (logits, labels), None,
                                                           batch, 0, 0)
    assert (tmp_path / "0_0.txt").read_text() == "".join(do.prediction_lines(ref.numpy(), batch["id"].numpy()))
    # weights changed in place -> engine reloads them
    with torch.no_grad():
        model.net.head.output_layer.bias.add_(1.0)
    logits2, _ = model.predict_step(batch, 1)
    assert ((logits2 - logits).cpu() - 1.0).abs().max() < 1e-5


def test_native_feeder_predict_loop(sd, tmp_path, golden_dir, built_lib):
    """BAM -> C++ feeder (pinned ring) -> clm_stage_ids on the copy stream -> clm_forward_staged -> prediction files:
    the same files as the Python data module + `run_predict`, and the labels the oracle gives for those batches."""
    from chimeralm_amd import bam, lm, predict as loop, tokenizer as T
    from chimeralm_amd.callbacks import PredictionWriter
    from chimeralm_amd.feeder import BamFeeder

    path = golden_dir / "test_chimric_reads.bam"
    device = torch.device("cuda", 0)
    model = lm.ChimeraLM.new(precision="fp32")
    model.load_state_dict(sd, strict=True)
    tok = T.CharTokenizer(model_max_length=2501, padding_side="left")
    dm = bam.BamDataModule(tokenizer=tok, predict_data_path=path, batch_size=10, max_predict_samples=25)
    dm.setup("predict")
    n_py = loop.run_predict(model, dm, PredictionWriter(tmp_path / "py"), device)
    with BamFeeder(path, batch_size=10, max_tokens=tok.max_len_single_sentence, max_reads=25, slots=2) as fd:
        n_nat = loop.run_predict_native(model, fd, PredictionWriter(tmp_path / "native"), device)
        assert fd.stats()["delivered"] == 25
    assert n_py == n_nat == 25
    names = sorted(p.name for p in (tmp_path / "py").iterdir())
    assert names == ["0_0.txt", "0_1.txt", "0_2.txt"] == sorted(p.name for p in (tmp_path / "native").iterdir())
    for n in names:
        assert (tmp_path / "py" / n).read_text() == (tmp_path / "native" / n).read_text()
    batch0 = next(iter(dm.predict_dataloader()))
    ref = ho.forward(batch0["input_ids"], sd).numpy()
    assert (tmp_path / "native" / "0_0.txt").read_text() == "".join(do.prediction_lines(ref, batch0["id"].numpy()))


def test_staging_api_state_machine(engines):
    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import EngineError

    e = engines["fp16"]
    ids = torch.from_numpy(_ids(3, 300)).pin_memory()
    k0 = e.stage_host_ids(ids.data_ptr(), N.DT_U8, ids.stride(0), 3, 300)
    k1 = e.stage_host_ids(ids.data_ptr(), N.DT_U8, ids.stride(0), 3, 300)
    assert {k0, k1} == {0, 1}
    with pytest.raises(EngineError, match="both staging buffers"):
        e.stage_host_ids(ids.data_ptr(), N.DT_U8, ids.stride(0), 3, 300)
    a, b = e.forward_staged(k0, 3), e.forward_staged(k1, 3)
    e.stage_wait(k0), e.stage_wait(k1)
    assert torch.equal(a.cpu(), b.cpu()) and torch.equal(a.cpu(), e.forward(ids.cuda()).cpu())
    with pytest.raises(EngineError, match="no batch staged"):
        e.forward_staged(k0, 3)


def test_error_behaviour(engines):
    from chimeralm_amd.engine import EngineError

    e = engines["fp32"]
    with pytest.raises(EngineError, match="max_seq_len"):
        e.forward(torch.zeros(1, 32771, dtype=torch.uint8).cuda())                       # beyond pos_emb rows (32770)
    with pytest.raises(EngineError):
        e.forward(torch.zeros(1, 9, dtype=torch.uint8))                                  # CPU tensor: no CPU path
    with pytest.raises(ValueError):
        e.forward(torch.zeros(1, 9, dtype=torch.float32).cuda())
    with pytest.raises(EngineError, match="shape"):
        e.load_weight("net.head.output_layer.bias", torch.zeros(3))
    with pytest.raises(EngineError, match="unknown"):
        e.load_weight("net.nope", torch.zeros(3))


@pytest.mark.parametrize("prec", ["fp32", "fp16c"])
def test_token_ids_outside_the_embedding_table_are_reported(engines, prec):
    """The reference raises IndexError inside nn.Embedding(16, 256) for such ids (hyena.py:249).  A kernel cannot raise: the id
    is clamped and the handle is flagged; clm_check (or the next forward) reports it once, then the engine is usable again."""
    from chimeralm_amd.engine import EngineError

    e = engines[prec]
    ids = _ids(2, 2100).astype(np.int64)
    good = e.forward(torch.from_numpy(ids).cuda()).cpu()
    e.check()
    bad = ids.copy()
    bad[1, 7] = 16
    e.forward(torch.from_numpy(bad).cuda())
    with pytest.raises(EngineError, match="token ids outside"):
        e.check()
    e.check()                                                           # reported once
    bad[1, 7] = -3
    e.forward(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    with pytest.raises(EngineError, match="token ids outside"):
        e.forward(torch.from_numpy(ids).cuda())                         # ... or by the next forward
    assert torch.equal(e.forward(torch.from_numpy(ids).cuda()).cpu(), good)


def test_cli_predict_then_filter_end_to_end(sd, tmp_path, golden_dir, built_lib):
    """`python -m chimeralm_amd predict BAM --weights DIR` (native feeder) writes the reference's prediction files, and
    `filter` consumes them: the two commands of the reference workflow (README: predict, then filter), as subprocesses."""
    import shutil
    import subprocess
    import sys

    from safetensors.torch import save_file

    wdir = tmp_path / "weights"
    wdir.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items() if not (k.endswith(".3.freq") or k.endswith(".5.freq"))},
              str(wdir / "model.safetensors"))                    # safetensors drops the aliases of the shared sine module
    bam = tmp_path / "reads.bam"
    shutil.copyfile(golden_dir / "test_chimric_reads.bam", bam)
    env = {**__import__("os").environ, "PYTHONPATH": str(REPO)}
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "predict", str(bam), "-g", "1", "-b", "25", "--weights", str(wdir),
                        "--precision", "fp16"], capture_output=True, text=True, env=env, cwd=str(REPO), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = bam.with_suffix(".predictions")
    files = sorted(out.glob("*.txt"))
    assert [f.name for f in files] == ["0_0.txt", "0_1.txt", "0_2.txt", "0_3.txt"]
    lines = [ln for f in files for ln in f.read_text().splitlines()]
    assert len(lines) == 100 and all(ln.split("\t")[1] in ("0", "1") for ln in lines)
    r = subprocess.run([sys.executable, "-m", "chimeralm_amd", "filter", str(bam), str(out), "-p"], capture_output=True, text=True,
                       env=env, cwd=str(REPO), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "predictions.txt").exists() and bam.with_suffix(".filtered.sorted.bam").exists()
    assert Path(str(bam.with_suffix(".filtered.sorted.bam")) + ".bai").exists()


def test_integration_md_ctypes_stub_runs_as_documented(sd, built_lib):
    """The ctypes binding printed in INTEGRATION.md section 3 is executed verbatim (only the library path is made absolute) and
    must give the same logits as the maintained binding."""
    import re

    from chimeralm_amd import lm

    text = (REPO / "INTEGRATION.md").read_text()
    block = next(b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "class HyenaDnaHip" in b)
    block = block.replace('C.CDLL("libchimeralm_hip.so")', f'C.CDLL("{built_lib}")')
    ns: dict = {}
    exec(compile(block, "INTEGRATION.md", "exec"), ns)  # noqa: S102
    model = lm.ChimeraLM.new(precision="fp16c")
    model.load_state_dict(sd, strict=True)
    stub = ns["HyenaDnaHip"](model.net, device=0)              # the stub's default: 3 = CLM_PREC_F16C
    ids = torch.from_numpy(_ids(3, 2500).astype(np.int64)).cuda()
    got = stub(ids)
    torch.cuda.synchronize()
    want = model.net(ids)
    assert torch.equal(got.cpu(), want.cpu())
