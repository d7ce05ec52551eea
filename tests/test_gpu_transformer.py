"""SequenceCNNTransformer on MI355X (csrc/tf_model.hip + attention.hip through the clm_tf_* C ABI) against the oracle
(oracle/transformer_oracle.py, pinned to the reference module by tests/golden/transformer_golden.npz)."""
import numpy as np
import pytest
import torch

from oracle import transformer_oracle as to

pytestmark = pytest.mark.gpu

# fp32 = the reference's arithmetic (exact-fp32 MFMA, csrc/tf_fp32.hip): held to north_star's gate, 1e-3 on the logits.
# fp16 / bf16 are the throughput modes of this net, REDUCED precision outside the gate: logits of the seeded classifier
# (scale 3) are 3..9 in magnitude, their bounds are ~0.5 % / 4 % of that; the encoder output (O(1) LayerNorm values) is
# checked separately.  fp16c (round 3: fp16 activations x hi + lo weights as on the Hyena path, and the attention output -- the one
# activation whose rounding does not average out over the positions -- as hi + lo planes) is 3e-5 .. 2.3e-4 from the oracle at logits
# of magnitude ~1 (scale 1) and 4.5e-4 .. 2e-3 at 5 .. 11 (scale 3: inside the gate from ~2,000 tokens up, outside for short reads);
# the module measures it on the loaded weights and falls back to fp16x3 (tests below).  Since round 5 fp16c is OPT-IN on this net:
# the module's and the yaml's default is fp16x3, which is inside the gate on every case.
GATE = 1e-3
TOL = {"fp32": GATE, "fp16x3": 1e-4, "fp16c": 1.2e-2, "fp16": 4e-2, "bf16": 4e-1}   # fp16x3 (round 4): a TENTH of the gate   # (fp16c: 9.6e-3 on the one-position read, <= 2.7e-3 otherwise)
TOL_HIDDEN = {"fp32": 2e-4, "fp16x3": 2e-4, "fp16c": 1e-2, "fp16": 1e-2, "bf16": 1e-1}


def _model(sd, prec, layers=12, selfcheck=False):
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=layers, precision=prec, selfcheck=selfcheck)
    assert set(net.state_dict()) == set(sd)                     # reference keys, `pos_encoder.pe` buffer included
    net.load_state_dict(sd, strict=True)
    return net


@pytest.mark.parametrize("prec,seed,B,L,pads", [("fp32", 0, 2, 1000, 0), ("fp32", 1, 3, 777, 40), ("fp32", 2, 1, 8, 0),
                                                ("fp32", 3, 2, 2055, 0), ("fp32", 4, 3, 4101, 7),
                                                ("fp16x3", 0, 2, 1000, 0), ("fp16x3", 1, 3, 777, 40), ("fp16x3", 2, 1, 8, 0),
                                                ("fp16x3", 3, 2, 2055, 0), ("fp16x3", 4, 3, 4101, 7),
                                                ("fp16", 0, 2, 1000, 0), ("fp16", 1, 3, 777, 40), ("fp16", 2, 1, 8, 0),
                                                ("fp16", 3, 2, 2055, 0), ("bf16", 0, 2, 1000, 0),
                                                ("fp16c", 0, 2, 1000, 0), ("fp16c", 1, 3, 777, 40), ("fp16c", 2, 1, 8, 0),
                                                ("fp16c", 3, 2, 2055, 0), ("fp16c", 4, 3, 4101, 7)])
def test_forward_matches_oracle(built_lib, golden_dir, prec, seed, B, L, pads):
    sd = to.make_state_dict(seed, to.PRODUCTION, scale=3.0)
    ids = to.synthetic_ids(100 + seed, B, L, pads)
    trace = {}
    ref = to.forward(torch.from_numpy(ids), sd, trace=trace).numpy()
    if (seed, B, L, pads) in ((0, 2, 1000, 0), (1, 3, 777, 40)):   # the very cases the reference module was run on
        g = np.load(golden_dir / "transformer_golden.npz")
        name = "prod" if seed == 0 else "prod_pad"
        assert np.abs(ref - g[f"{name}_logits"]).max() < 5e-5
    net = _model(sd, prec)
    got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    L3 = L // 8
    hid = net.debug_fetch("hidden", (B, L3, 256))
    err_h = np.abs(hid - trace["layer11"].numpy()).max()
    err = np.abs(got - ref).max()
    print(f"{prec} B={B} L={L}: |logits - oracle| = {err:.2e}, |hidden - oracle| = {err_h:.2e}")
    assert err < TOL[prec] and err_h < TOL_HIDDEN[prec], f"{prec}: |logits - oracle| = {err:.2e} (hidden {err_h:.2e})"
    decided = np.abs(ref[:, 0] - ref[:, 1]) > (2 if prec in ("fp32", "fp16x3") else 4) * TOL[prec]
    assert (got.argmax(1)[decided] == ref.argmax(1)[decided]).all()
    pooled = net.debug_fetch("pooled", (B, 256))
    assert np.abs(pooled - trace["pooled"].numpy()).max() < TOL_HIDDEN[prec]
    if prec == "fp16x3":        # the handle's own referee pass (its exact-fp32 kernels): what the mode is off by on these ids
        from chimeralm_amd import _native as N
        d = net._measure(N.load(), "test", torch.from_numpy(ids).cuda())
        print(f"fp16x3 B={B} L={L}: clm_tf_selfcheck |fp16x3 - exact fp32| = {d:.2e}")
        assert 0 < d <= TOL[prec]
    # ids as uint8 with a row stride give the same bits
    wide = torch.zeros((B, L + 5), dtype=torch.uint8).cuda()
    wide[:, :L] = torch.from_numpy(ids.astype(np.uint8)).cuda()
    assert torch.equal(net(wide[:, :L]).cpu(), torch.from_numpy(got))
    net.close()


@pytest.mark.parametrize("seed,B,L,pads", [(0, 2, 1000, 0), (1, 3, 777, 40), (2, 1, 8, 0), (5, 5, 520, 3), (6, 2, 4101, 0)])
def test_fused_fp32_encoder_equals_the_separate_kernels(built_lib, monkeypatch, seed, B, L, pads):
    """Exact fp32 runs the dense layers of an encoder layer and the attention on the fp32 MFMA in fused kernels since round 4
    (tail32.hip enc32_kernel; tf_fp32.hip).  Against the separate launches of round 2 (CLM_DEBUG=unfused_fp32): the same fp32
    products in another summation order -- logits and the encoder output agree to fp32 rounding; one-tile, ragged-tile and padded cases."""
    sd = to.make_state_dict(seed, to.PRODUCTION, scale=3.0)
    ids = torch.from_numpy(to.synthetic_ids(300 + seed, B, L, pads)).cuda()
    a_net = _model(sd, "fp32")
    a = a_net(ids).cpu().numpy()
    ha = a_net.debug_fetch("hidden", (B, L // 8, 256)).copy()
    a_net.close()
    monkeypatch.setenv("CLM_DEBUG", "unfused_fp32")      # read by clm_tf_create
    b_net = _model(sd, "fp32")
    b = b_net(ids).cpu().numpy()
    hb = b_net.debug_fetch("hidden", (B, L // 8, 256)).copy()
    b_net.close()
    monkeypatch.delenv("CLM_DEBUG")
    print(f"tf fp32 fused vs separate, {B} x {L}: |dlogit| {np.abs(a - b).max():.2e}, |dhidden| {np.abs(ha - hb).max():.2e} of {np.abs(hb).max():.3g}")
    assert np.abs(a - b).max() <= 1e-4 and np.abs(ha - hb).max() <= 2e-5 * max(1.0, float(np.abs(hb).max()))


@pytest.mark.parametrize("prec", ["fp16c", "fp32"])
def test_more_shorter_reads_after_a_long_batch_regrow_the_pooled_buffer(built_lib, prec):
    """`pooled` is [B][256] and scales with B alone; 4 x 4096 then 16 x 512 on ONE handle fits every token / row
    capacity of the first call, so only a capacity of its own regrows it (pool_head_kernel wrote past 4 rows before)."""
    sd = to.make_state_dict(5, to.PRODUCTION, scale=1.0)
    net = _model(sd, prec, selfcheck=False)
    net(torch.from_numpy(to.synthetic_ids(7, 4, 4096, 0)).cuda())
    ids = to.synthetic_ids(8, 16, 512, 3)
    trace = {}
    ref = to.forward(torch.from_numpy(ids), sd, trace=trace).numpy()
    got = net(torch.from_numpy(ids).cuda()).cpu().numpy()
    pooled = net.debug_fetch("pooled", (16, 256))
    assert np.abs(pooled - trace["pooled"].numpy()).max() < TOL_HIDDEN[prec]
    assert np.abs(got - ref).max() < (GATE if prec == "fp32" else TOL[prec])
    fresh = _model(sd, prec, selfcheck=False)                   # same bits as a handle that never saw the long batch
    assert np.array_equal(fresh(torch.from_numpy(ids).cuda()).cpu().numpy(), got)
    fresh.close()
    net.close()


TWO_LAYERS = to.Config(max_len=512, num_encoder_layers=2)


def _two_layers(sd, prec):
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(vocab_size=12, max_len=TWO_LAYERS.max_len, num_encoder_layers=2, precision=prec, selfcheck=False)
    net.load_state_dict(sd, strict=True)
    return net


@pytest.mark.parametrize("prec", ["fp16c", "fp32", "fp16x3"])
def test_workspace_follows_a_sequence_of_shapes(built_lib, prec):
    """Every workspace buffer grows on its own and none is ever reset: 2 x 1000, 9 x 64, 1 x 2048, 2 x 1000 tokens on ONE handle,
    each batch bit for bit what a fresh handle computes.  The family of the `pooled` overrun at its smallest sizes: 9 > 2 reads with
    fewer tokens and rows than the first batch (only the per-read buffers regrow); 64 tokens are L3 = 8 positions, one tile;
    1 x 2048 has about the tokens of 2 x 1000 in one read (every buffer regrows a little, next to `pooled`, which does not); the last
    batch runs in buffers that are all larger than it needs."""
    sd = to.make_state_dict(9, TWO_LAYERS, scale=1.0)
    net = _two_layers(sd, prec)
    for seed, (B, L) in enumerate([(2, 1000), (9, 64), (1, 2048), (2, 1000)]):
        ids = torch.from_numpy(to.synthetic_ids(900 + seed, B, L, 3)).cuda()
        got = net(ids).cpu()
        fresh = _two_layers(sd, prec)
        want = fresh(ids).cpu()
        fresh.close()
        assert torch.isfinite(want).all() and torch.equal(got, want), f"{prec}: batch {seed} ({B} x {L}) differs from a fresh handle's"
    net.close()


def test_run_mode_survives_a_selfcheck(built_lib):
    """clm_tf_selfcheck runs whole forwards in the handle's mode and in exact fp32 whatever the fall-back level and the debug stop
    say -- and leaves both as it found them: afterwards the handle still reports fp16x3 (fp16c at fall-back level 1), a forward
    still ends behind pe_ln, and with the stop cleared it computes what a handle that never ran a self-check does."""
    from chimeralm_amd import _native as N
    from chimeralm_amd.transformer import TransformerEngineError

    sd = to.make_state_dict(10, TWO_LAYERS, scale=1.0)
    ids = torch.from_numpy(to.synthetic_ids(910, 2, 64, 0)).cuda()
    net, plain = _two_layers(sd, "fp16c"), _two_layers(sd, "fp16c")
    lib = N.load()
    for m in (net, plain):
        m(ids)                                                  # (creates the engine)
        m._check(lib.clm_tf_set_fallback(m._h, 1))
    net.debug_stop_after("pe_ln")
    diff, differ = net._selfcheck_call(lib, ids)
    assert np.isfinite(diff) and diff > 0                       # whole forwards of the MODE against exact fp32 ran
    assert net._arith(lib) == "fp16x3"
    net(ids)
    with pytest.raises(TransformerEngineError, match="did not produce"):
        net.debug_fetch("scores", (2, 8))
    net.debug_stop_after(None)
    assert torch.equal(net(ids).cpu(), plain(ids).cpu())
    net.close()
    plain.close()


def test_arguments_and_errors(built_lib):
    from chimeralm_amd.transformer import SequenceCNNTransformer, TransformerEngineError

    with pytest.raises(NotImplementedError):
        SequenceCNNTransformer(vocab_size=12, max_len=64, d_model=128)
    net = SequenceCNNTransformer(vocab_size=12, max_len=16, num_encoder_layers=1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros((1, 64), dtype=torch.int64))
    with pytest.raises(TransformerEngineError, match="Sequence too long"):     # transformer.py:21 asserts the same
        net(torch.full((1, 8 * 17), 7, dtype=torch.int64).cuda())
    with pytest.raises(TransformerEngineError, match="L >= 8"):
        net(torch.full((1, 7), 7, dtype=torch.int64).cuda())
    out = net(torch.full((2, 128), 7, dtype=torch.int64).cuda())
    assert out.shape == (2, 2) and torch.isfinite(out).all()
    net.close()
    small = SequenceCNNTransformer(vocab_size=12, max_len=16, num_encoder_layers=1, precision="fp16c")   # guarded by default:
    out = small(torch.full((2, 128), 7, dtype=torch.int64).cuda())          # its seeded sample must respect max_len (8 * 16 tokens)
    assert small.selfcheck_report["samples"][0]["sample"] == "synthetic 4 x 128" and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="precision must be"):
        SequenceCNNTransformer(vocab_size=12, max_len=16, precision="fp8")
    small.close()


@pytest.mark.parametrize("seed,B,L", [(0, 2, 1000), (1, 2, 2055), (2, 2, 4101), (3, 2, 8193)])
def test_fp16c_is_inside_the_gate_at_unit_logits(built_lib, seed, B, L):
    """Weights at scale 1 (logits of magnitude 0.5 .. 1.3): the compensated mode's raw error stays well under the reference's 1e-3
    (3e-5 .. 2.3e-4 measured) where plain fp16 is at 5e-4 .. 3e-3 -- and the guard keeps the mode."""
    sd = to.make_state_dict(seed, to.PRODUCTION, scale=1.0)
    ids = to.synthetic_ids(100 + seed, B, L)
    ref = to.forward(torch.from_numpy(ids), {k: v.double() for k, v in sd.items()}, dtype=torch.float64).numpy()
    dev = torch.from_numpy(ids).cuda()
    raw = _model(sd, "fp16c")
    got = raw(dev).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"fp16c scale 1 seed {seed} L={L}: |logits - oracle| = {err:.2e} (|logit| max {np.abs(ref).max():.2f})")
    assert err < 0.4 * GATE
    assert (got.argmax(1) == ref.argmax(1))[np.abs(ref[:, 0] - ref[:, 1]) > 2 * GATE].all()
    raw.close()
    guarded = _model(sd, "fp16c", selfcheck=True)
    got_g = guarded(dev).cpu().numpy().astype(np.float64)
    rep = guarded.selfcheck_report
    assert rep["fallback"] is False and rep["max_abs_dlogit"] <= rep["tol"] == 5e-4 and np.array_equal(got_g, got)
    guarded.close()


def test_selfcheck_falls_back_to_fp16x3_and_the_abi_agrees(built_lib):
    """Weights at scale 3, 1,000-token reads (logits ~5): the mode is 2e-3 off, the module measures that through `clm_tf_selfcheck`,
    falls back -- round 5: to fp16x3, the next-fastest arithmetic inside the gate, not to the slowest -- and from then on returns an
    fp16x3 engine's bits; the C entry's figure is the difference of the two modes; level 2 of the C entry is exact fp32."""
    import ctypes as C

    from chimeralm_amd import _native as N

    sd = to.make_state_dict(0, to.PRODUCTION, scale=3.0)
    ids = torch.from_numpy(to.synthetic_ids(100, 3, 1000)).cuda()
    exact = _model(sd, "fp32")
    want = exact(ids).cpu()
    x3 = _model(sd, "fp16x3")
    want_x3 = x3(ids).cpu()
    assert (want_x3 - want).abs().max().item() < 1e-4 and not torch.equal(want_x3, want)
    raw = _model(sd, "fp16c")
    got_raw = raw(ids).cpu()
    lib = N.load()
    diff, differ = C.c_float(), C.c_int()
    assert lib.clm_tf_selfcheck(raw._h, C.c_void_p(ids.data_ptr()), N.DT_I64, ids.stride(0), 3, 1000, None, C.byref(diff),
                                C.byref(differ)) == 0
    mine = (got_raw - want).abs().max().item()
    print(f"clm_tf_selfcheck: {diff.value:.3e}; |fp16c - fp32| of two handles: {mine:.3e}")
    assert abs(diff.value - mine) < 1e-6 and diff.value > 5e-4 and differ.value == 0
    assert torch.equal(raw(ids).cpu(), got_raw)                  # the check leaves the mode as it was
    assert lib.clm_tf_set_fallback(raw._h, 1) == 0                # level 1: the fp32-path kernels on hi + lo halfs
    assert torch.equal(raw(ids).cpu(), want_x3)
    assert lib.clm_tf_selfcheck(raw._h, C.c_void_p(ids.data_ptr()), N.DT_I64, ids.stride(0), 3, 1000, None, C.byref(diff),
                                C.byref(differ)) == 0 and abs(diff.value - mine) < 1e-6      # the MODE is on trial, whatever the level
    assert lib.clm_tf_set_fallback(raw._h, 2) == 0                # level 2: exact fp32
    assert torch.equal(raw(ids).cpu(), want)
    assert lib.clm_tf_set_fallback(raw._h, 3) != 0
    assert lib.clm_tf_set_fallback(raw._h, 0) == 0
    assert torch.equal(raw(ids).cpu(), got_raw)
    # an fp16x3 handle: level 1 = its own exact kernels (the switch did nothing on such a handle)
    assert lib.clm_tf_set_fallback(x3._h, 1) == 0 and torch.equal(x3(ids).cpu(), want)
    assert lib.clm_tf_set_fallback(x3._h, 0) == 0 and torch.equal(x3(ids).cpu(), want_x3)
    # an fp32 handle reports 0 / 0
    assert lib.clm_tf_selfcheck(exact._h, C.c_void_p(ids.data_ptr()), N.DT_I64, ids.stride(0), 3, 1000, None, C.byref(diff),
                                C.byref(differ)) == 0 and diff.value == 0.0 and differ.value == 0
    raw.close()
    guarded = _model(sd, "fp16c", selfcheck=True)
    with pytest.warns(RuntimeWarning, match="falling back to fp16x3"):
        got = guarded(ids).cpu()
    rep = guarded.selfcheck_report
    assert rep["fallback"] is True and rep["fallback_precision"] == "fp16x3" and rep["max_abs_dlogit"] > rep["tol"] == 5e-4
    assert torch.equal(got, want_x3) and torch.equal(guarded(ids[:2, :499]).cpu(), x3(ids[:2, :499]).cpu())
    guarded.load_state_dict(to.make_state_dict(0, to.PRODUCTION, scale=0.25), strict=True)   # new weights: on trial again
    guarded(ids)
    assert guarded.selfcheck_report["fallback"] is False
    guarded.close()
    exact.close()
    x3.close()
    from chimeralm_amd.transformer import SequenceCNNTransformer
    assert SequenceCNNTransformer(vocab_size=12, max_len=16).precision == "fp16x3"     # the module default is a mode inside the gate


def test_random_shapes_fp16c_against_the_exact_kernels(built_lib):
    """Sixteen seeded (reads, tokens) shapes through one fp16c model against the exact-fp32 kernels of the same handle
    (`clm_tf_selfcheck`): positions on and off the 128-row tile boundary, single-position reads, odd batches -- the two-plane
    attention output and the two-pass out_proj must index them all."""
    import ctypes as C

    from chimeralm_amd import _native as N

    sd = to.make_state_dict(5, to.PRODUCTION, scale=1.0)
    net = _model(sd, "fp16c")
    lib = N.load()
    rng = np.random.default_rng(7)
    lengths = [8, 15, 16, 1023, 1024, 1025, 1031, 2055, 4101] + [int(x) for x in rng.integers(8, 6000, size=7)]
    worst = 0.0
    for k, L in enumerate(lengths):
        B = int(rng.integers(1, 6))
        ids = torch.from_numpy(to.synthetic_ids(300 + k, B, L, pads=(L // 4 if k % 2 else 0))).cuda()
        out = net(ids)
        assert torch.isfinite(out).all()
        diff, differ = C.c_float(), C.c_int()
        assert lib.clm_tf_selfcheck(net._h, C.c_void_p(ids.data_ptr()), N.DT_I64, ids.stride(0), B, L, None, C.byref(diff),
                                    C.byref(differ)) == 0
        worst = max(worst, diff.value)
        assert diff.value < (GATE if L >= 512 else 4e-3), f"{B} x {L}: |fp16c - exact fp32| = {diff.value:.2e}"
    print(f"16 random shapes: worst |fp16c - exact fp32| = {worst:.2e}")
    net.close()


_LONG_ORACLE: dict = {}


def _long_case(seed, B, L):
    """Weights, ids (reads 1 and 2 of the padded case left-padded by different runs) and the oracle's logits, encoder output and
    pooled vector, one read at a time (the score matrices of one read take ~0.5 GB per layer); shared by fp32 and fp16x3."""
    if (seed, B, L) not in _LONG_ORACLE:
        sd = to.make_state_dict(seed, to.PRODUCTION, scale=3.0)
        ids = to.synthetic_ids(200 + seed, B, L)
        if L % 8:                                              # the ragged case: [PAD] runs as the collator leaves them
            ids[1, :900] = 4
            ids[2, :5000] = 4
        outs = []
        for r in range(B):
            trace = {}
            logit = to.forward(torch.from_numpy(ids[r: r + 1]), sd, trace=trace)
            outs.append((logit.numpy(), trace["layer11"].numpy(), trace["pooled"].numpy()))
        _LONG_ORACLE[(seed, B, L)] = (sd, ids, *(np.concatenate(x) for x in zip(*outs)))
    return _LONG_ORACLE[(seed, B, L)]


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("seed,B,L", [(7, 2, 32768), (8, 3, 32700), (9, 3, 8003)])
def test_long_context_matches_oracle(built_lib, prec, seed, B, L):
    """The checks of `test_forward_matches_oracle` at the benched context: 4,096 attention positions (32 query tiles, whole key
    tiles), 4,087 (32 query tiles, ragged last key tile, padded reads) and 1,000 (8 query tiles, ragged)."""
    sd, ids, ref, ref_h, ref_p = _long_case(seed, B, L)
    net = _model(sd, prec)
    t = torch.from_numpy(ids).cuda()
    got = net(t).cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    err_h = np.abs(net.debug_fetch("hidden", (B, L // 8, 256)) - ref_h).max()
    err_p = np.abs(net.debug_fetch("pooled", (B, 256)) - ref_p).max()
    msg = f"{prec} B={B} L={L} ({L // 8} positions): |logits - oracle| = {err:.2e}, |hidden - oracle| = {err_h:.2e}, |pooled| {err_p:.2e}"
    if prec == "fp16x3":
        from chimeralm_amd import _native as N
        d = net._measure(N.load(), "test", t)
        msg += f", clm_tf_selfcheck {d:.2e}"
        assert 0 < d <= TOL[prec], msg
    print(msg)
    assert err < TOL[prec] and err_h < TOL_HIDDEN[prec] and err_p < TOL_HIDDEN[prec], msg
    decided = np.abs(ref[:, 0] - ref[:, 1]) > 2 * TOL[prec]
    assert (got.argmax(1)[decided] == ref.argmax(1)[decided]).all()
    net.close()


_LONG_FP32: dict = {}


@pytest.mark.parametrize("prec", ["fp16c", "fp16", "bf16"])
def test_16bit_modes_at_long_context(built_lib, prec):
    """The 16-bit modes at the net's long-context shape, 2 x 32,768 bp = 4,096 attention positions (32 query tiles, 64 key tiles of
    attention_fwd_kernel; elsewhere they stop at 512 positions): logits and the `hidden` tap against an fp32 handle on the same
    weights and ids -- the very handle `test_long_context_matches_oracle[7-2-32768-fp32]` ties to the oracle at this shape -- within
    the file's own TOL and TOL_HIDDEN."""
    B, L = 2, 32768
    sd = to.make_state_dict(7, to.PRODUCTION, scale=3.0)                          # weights and ids of `_long_case(7, 2, 32768)`
    t = torch.from_numpy(to.synthetic_ids(207, B, L)).cuda()
    if not _LONG_FP32:
        exact = _model(sd, "fp32")
        _LONG_FP32["logits"] = exact(t).cpu().numpy()
        _LONG_FP32["hidden"] = exact.debug_fetch("hidden", (B, L // 8, 256)).copy()
        exact.close()
    net = _model(sd, prec)
    got = net(t).cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - _LONG_FP32["logits"]).max()
    err_h = np.abs(net.debug_fetch("hidden", (B, L // 8, 256)) - _LONG_FP32["hidden"]).max()
    net.close()
    msg = f"{prec} B={B} L={L} (4,096 positions): |logits - fp32 handle| = {err:.2e}, |hidden - fp32 handle| = {err_h:.2e}"
    print(msg)
    assert err < TOL[prec] and err_h < TOL_HIDDEN[prec], msg


def test_fp16x3_bench_line_rows_are_independent(built_lib):
    """The benched transformer line, 32 x 32,768 in fp16x3 (4,096 positions through attention_x3_kernel): bit-identical on a second
    run, rows run alone equal their batch rows bit for bit (no operation mixes reads), and exact fp32 agrees on all 32 rows."""
    sd = to.make_state_dict(0, to.PRODUCTION, scale=3.0)
    t = torch.from_numpy(to.synthetic_ids(110, 32, 32768)).cuda()
    net = _model(sd, "fp16x3")
    a = net(t).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, net(t).cpu())
    for r in (0, 15, 31):
        assert torch.equal(net(t[r: r + 1]).cpu(), a[r: r + 1]), f"row {r} alone differs from its batch row"
    exact = _model(sd, "fp32")
    d = (exact(t).cpu() - a).abs().max().item()
    print(f"transformer fp16x3 32 x 32768: every row vs exact fp32 {d:.2e}")
    assert d <= 1e-4
    exact.close()
    net.close()


@pytest.mark.parametrize("key", ["transformer_encoder.layers.3.linear1.weight", "cnn.3.weight"])
def test_fp16x3_weight_range_of_the_transformer(built_lib, caplog, key):
    """fp16x3 packs weights x 2^10 as fp16 halfs, which saturate at |w| >= 64: with one encoder or CNN-stem weight at 300 the default
    module runs exact fp32, within fp16x3's bound of the oracle, warns and records it; an fp16c model that falls back names exact
    fp32 as what it falls back to."""
    from chimeralm_amd.transformer import SequenceCNNTransformer

    sd = to.make_state_dict(0, to.PRODUCTION, scale=3.0)
    sd[key].view(-1)[1234] = 300.0
    ids = to.synthetic_ids(100, 2, 1000)
    ref = to.forward(torch.from_numpy(ids), sd).numpy()
    t = torch.from_numpy(ids).cuda()
    net = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=12)
    net.load_state_dict(sd, strict=True)
    with caplog.at_level("WARNING", logger="chimeralm_amd"):
        got = net(t).cpu().numpy()
    rep = net.precision_report
    assert rep["precision"] == "fp16x3" and rep["fallback"] is True and rep["fallback_precision"] == "fp32" and rep["max_abs_weight"] == 300.0
    assert any("exact-fp32" in r.getMessage() for r in caplog.records)
    err = np.abs(got - ref).max()
    print(f"transformer fp16x3 with {key} = 300: |logits - oracle| {err:.2e}")
    assert err <= TOL["fp16x3"]
    net.close()
    fc = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=12, precision="fp16c", selfcheck_tol=1e-12)
    fc.load_state_dict(sd, strict=True)
    with pytest.warns(RuntimeWarning, match="falling back to exact fp32"):
        got_c = fc(t).cpu().numpy()
    assert fc.precision_report["fallback_precision"] == "fp32"
    assert fc.selfcheck_report["fallback"] is True and fc.selfcheck_report["fallback_precision"] == "fp32"
    assert np.abs(got_c - ref).max() <= TOL["fp16x3"]
    fc.close()
