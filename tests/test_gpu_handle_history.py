"""GPU (MI355X): a handle WITH A HISTORY against a fresh one.

Every parity test builds a handle, loads one set of weights and runs.  The product keeps ONE engine handle per module for its
lifetime, reloads weights into it whenever a parameter changes, and flips it between arithmetics while batches run.  Each handle
carries state that is a function of the weights or of those switches (packings, `ztab`, `fir`, the filter sets per length class,
the [PAD] tables, `x3_wmax`; `packed["x3.*"]` of the transformer; the block-0 table and BatchNorm scale / shift of the CNN), and a
piece of it that survives a reload gives plausible, finite, wrong logits.

The reference for "a handle with a history" is not a tolerance: every engine here is bitwise deterministic and a result does not
depend on the workspace it ran in, so it is A FRESH HANDLE -- same configuration, loaded once with the final weights, put into the
final switch state, run through the same probe batches in the same order -- and the assertion is `np.array_equal`.

One carve-out (csrc/clm_api.hip ensure_pad_table): a [PAD] table is built for a length CLASS and its values differ between
classes by the rounding of the transform size, so the fresh handle runs the same probe sequence from the first probe on (the
long padded probe comes FIRST: both handles then build the same classes in the same order).  Warm-up batches run only on the
handle under test and only BEFORE the event.

Each scenario also has an anchor (the short probes are within the neighbouring test files' per-mode bound of the oracle / fp64
forward; the constants are restated below) and a non-vacuity check: EVERY probe moved by more than 10x that bound between before
and after a weight event.  For a SWITCH between two arithmetics that factor cannot hold -- both sides are within the bound of the
same oracle, so they are at most twice the bound apart -- and the check there is that the bits changed at all where the
arithmetic did.  Every scenario prints one line: what changed, max |before - after|, "== fresh"."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import cnn_reference as cr
import mamba_reference as mr
from oracle import hyena_oracle as ho
from oracle import transformer_oracle as to

pytestmark = pytest.mark.gpu

GATE = 1e-3
H_TOL = {"fp32": GATE, "fp16c": GATE, "fp16x3": 1e-4, "fp16": 5e-3, "bf16": 6e-2}      # tests/test_gpu_parity.py TOL
TF_TOL = {"fp32": GATE, "fp16x3": 1e-4, "fp16c": 1.2e-2, "fp16": 4e-2, "bf16": 4e-1}   # tests/test_gpu_transformer.py TOL
CNN_TOL = 1e-4                                                                          # tests/test_gpu_cnn.py TOL
MAMBA_TOL = 1e-4                                                                        # tests/test_gpu_mamba.py TOL
BB, HD = ho.BB, ho.HD


# ------------------------------------------------------------------------------------------------ shared helpers
def _run(handle, probes):
    return [handle(t).cpu().numpy() for t in probes]


def _maxdiff(a, b):
    """Largest |a - b| of each probe."""
    return [float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) for x, y in zip(a, b)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_same_as_fresh(make_handle, final_sd, final_switches, probes, got, what="", run=_run):
    """`got` = the probe results of the handle under test.  A fresh handle from `make_handle()`, loaded once with `final_sd`, put
    into its state by `final_switches(handle)` (or None), runs `probes` in the same order: equal bit for bit.  Returns its results.
    `run(handle, probes)` is what produced `got` (the logits of every probe unless a scenario also looks at an intermediate)."""
    fresh = make_handle()
    try:
        fresh.load_state_dict(final_sd)
        if final_switches is not None:
            final_switches(fresh)
        want = run(fresh, probes)
    finally:
        fresh.close()
    bad = {i: d for i, d in enumerate(_maxdiff(got, want)) if not np.array_equal(got[i], want[i])}
    assert not bad, f"{what}: probes {sorted(bad)} differ from a fresh handle's (max |d| per probe {bad})"
    return want


def _moved(before, after, bound, what, every=True):
    """Non-vacuity of a weight event: every probe (or, `every=False`, some probe) moved by more than 10x the mode's bound."""
    d = _maxdiff(before, after)
    print(f"{what}: max |before - after| {max(d):.2e} (least-moved probe {min(d):.2e}, needed > {10 * bound:.1e}), == fresh")
    assert (min(d) if every else max(d)) > 10 * bound, f"{what}: the event did not move the probes: {d} (needed > {10 * bound:.1e})"


def _tensor(net, key):
    """The parameter or buffer of `net` that `state_dict()[key]` shows."""
    try:
        return net.get_parameter(key)
    except AttributeError:
        return net.get_buffer(key)


def _clone(sd):
    return {k: v.detach().clone() for k, v in sd.items()}


# ================================================================================================ 1. Hyena, C ABI (Engine)
def _plain(B, L, seed):
    ids, _ = ho.synthetic_batch(seed, B, L - 1, seed=4321)
    return ids


def _padded(L, prefixes, seed):                                  # as tests/test_gpu_pad_prefix.py::_padded_batch
    rng = np.random.default_rng(seed)
    ids = rng.integers(7, 11, size=(len(prefixes), L)).astype(np.uint8)
    ids[:, -1] = 1
    for b, p in enumerate(prefixes):
        ids[b, :p] = 4
    return ids


_PLAIN_SHAPES = ((3, 300), (2, 1025), (2, 6000), (2, 8193), (2, 16385), (3, 20000))
_PAD_LONG = (20000, (19000, 16500, 8320, 100))
_PAD_SHORT = (3000, (2944, 2000, 0))


def _batches(seed0):
    """Every cache kind: a short read, the peeled last token, the 16,384-point class with lane-packed spectra, 8,193, long reads with
    reversed filters, and two left-padded batches (segment spectra and `dots` of the long [PAD] table).  The long padded one first."""
    out = [_padded(*_PAD_LONG, seed=seed0), _padded(*_PAD_SHORT, seed=seed0 + 1)]
    out += [_plain(B, L, seed0 + 2 + i) for i, (B, L) in enumerate(_PLAIN_SHAPES)]
    return out


_SHORT = (1, 2, 3)                                               # probes the oracle is run on: 3 x 3,000 padded, 3 x 300, 2 x 1,025


@pytest.fixture(scope="module")
def hy(built_lib):
    warm_np, probe_np = _batches(7000), _batches(8000)
    return {"warm": [torch.from_numpy(x).cuda() for x in warm_np], "probes": [torch.from_numpy(x).cuda() for x in probe_np],
            "probe_np": probe_np, "A": ho.make_state_dict(0, head_scale=3.0), "B": ho.make_state_dict(3, head_scale=3.0)}


_ORACLE: dict = {}


def _hy_anchor(hy, got, sd, sd_name, bound, what, short_only=False, forced16=False):
    """The short probes against the fp32 oracle on `sd` (cached under `sd_name`).  `forced16`: fp16c with its length switch forced
    to 1 runs the 16-bit kernels on reads the product never gives them unmeasured -- their error grows like 1 / sqrt(L), which is why
    the switch exists, and tests/test_gpu_parity.py holds them to the gate below 2,048 tokens on draw 0 only (this file measured
    1.10e-3 on the 300-token probe after the score-slot edit, equal to a fresh handle's) -- so there the anchor is the probe from
    2,048 tokens up; the shorter ones are printed."""
    if sd_name not in _ORACLE:
        _ORACLE[sd_name] = [ho.forward(torch.from_numpy(hy["probe_np"][i].astype(np.int64)), sd).numpy() for i in _SHORT]
    picked = got if short_only else [got[i] for i in _SHORT]
    per_probe = _maxdiff(picked, _ORACLE[sd_name])
    if forced16:
        print(f"{what}: 16-bit kernels forced below the default switch, |logits - oracle| per short probe {per_probe}")
        per_probe = [d for d, i in zip(per_probe, _SHORT) if hy["probe_np"][i].shape[1] >= 2048]
    err = max(per_probe)
    print(f"{what}: short probes |logits - oracle| {err:.2e} (bound {bound:.0e})")
    assert err <= bound, f"{what}: |logits - oracle| {err:.2e} > {bound}"


def _min1(e):
    e.set_f16c_min_len(1)


def _min1_mlp(e):
    e.set_f16c_min_len(1)
    e.set_mlp_compensation(True)


# name -> (handle precision, switches put on after the first load, bound)
H_MODES = {"fp32": ("fp32", None), "fp16x3": ("fp16x3", None), "fp16c@1": ("fp16c", _min1), "fp16c": ("fp16c", None),
           "fp16c@1+mlp": ("fp16c", _min1_mlp), "fp16": ("fp16", None), "bf16": ("bf16", None)}


def _maker(prec):
    def make():
        from chimeralm_amd.engine import Engine

        return Engine("cuda:0", precision=prec, chunk_reads=4)
    return make


def _warmed(hy, mode, sd):
    """A handle with draw `sd`, its mode's switches, every warm-up batch run, and the probe results on those weights."""
    prec, switches = H_MODES[mode]
    e = _maker(prec)()
    e.load_state_dict(sd)
    if switches:
        switches(e)
    short = mode == "bf16"
    for t in (hy["warm"][i] for i in (_SHORT if short else range(len(hy["warm"])))):
        e.forward(t)
    probes = [hy["probes"][i] for i in _SHORT] if short else hy["probes"]
    return e, switches, probes, _run(e, probes)


@pytest.mark.parametrize("mode", list(H_MODES))
def test_hyena_full_reload(hy, mode):
    """Draw A, every warm-up batch, then draw B into the same handle: the probes equal a fresh handle's with B.  (ABI level: the
    switches set after the first load stay over `clm_finalize`, so the handle under test is not told them again.)"""
    prec = H_MODES[mode][0]
    e, switches, probes, before = _warmed(hy, mode, hy["A"])
    try:
        e.load_state_dict(hy["B"])
        after = _run(e, probes)
        assert_same_as_fresh(_maker(prec), hy["B"], switches, probes, after, f"hyena {mode} A -> B")
        _moved(before, after, H_TOL[prec], f"hyena {mode}: full reload, draw 0 -> draw 3")
        _hy_anchor(hy, after, hy["B"], "B", H_TOL[prec], f"hyena {mode} after the reload", short_only=mode == "bf16")   # (all short probes, forced modes too)
    finally:
        e.close()


# One case per derived structure (keys as in csrc/clm_api.hip expected_keys), applied cumulatively.  The factors are chosen so
# that every probe moves by more than 10x the mode's bound.
_EDITS = [
    (BB + "embeddings.word_embeddings.weight", lambda w: -w, "ztab, [PAD] tables"),
    (BB + "layers.0.norm1.weight", lambda w: 0.5 * w.flip(0), "ztab"),
    (BB + "layers.0.mixer.in_proj.bias", lambda w: -w + 0.25, "ztab, fir"),
    (BB + "layers.1.mixer.short_filter.weight", lambda w: -w, "fir"),
    (BB + "layers.0.mixer.filter_fn.implicit_filter.6.weight", lambda w: -w, "ktime, kf, kfp, krev, long partition spectra"),
    (BB + "layers.2.mixer.filter_fn.bias", lambda w: -2.0 * w, "filter bias"),
    (BB + "layers.3.mixer.filter_fn.modulation.deltas", lambda w: 0.1 * w, "filter modulation"),
    (BB + "layers.1.mixer.out_proj.weight", lambda w: -w, "all packings"),
    (BB + "layers.0.mlp.fc1.weight", lambda w: -w, "pk_mode as plain fp16, pk_mlpc"),
    (HD + "attention.0.weight", lambda w: -w, "the score slot"),
    (HD + "classifier.3.weight", lambda w: -w, "head_t"),
    (BB + "ln_f.bias", lambda w: w + 1.0, "ln_f"),
]


@pytest.mark.parametrize("mode", ["fp16c@1", "fp16c@1+mlp", "fp32", "fp16x3"])
def test_hyena_one_key_at_a_time(hy, mode):
    """After the warm-up on draw A, ONE tensor through `load_weight` + `finalize`, then the probes: a fresh handle loaded with the
    edited state dict gives the same bits.  One warmed handle per mode, the edits cumulative."""
    prec = H_MODES[mode][0]
    e, switches, probes, before = _warmed(hy, mode, hy["A"])
    sd = _clone(hy["A"])
    try:
        for n, (key, edit, derived) in enumerate(_EDITS):
            sd[key] = edit(sd[key]).contiguous()
            e.load_weight(key, sd[key])
            e.finalize()
            after = _run(e, probes)
            what = f"hyena {mode}: {key.split('backbone.')[-1]} ({derived})"
            assert_same_as_fresh(_maker(prec), sd, switches, probes, after, what)
            _moved(before, after, H_TOL[prec], what)
            _hy_anchor(hy, after, sd, f"edit{n}", H_TOL[prec], what, forced16=mode.startswith("fp16c@1"))
            before = after
    finally:
        e.close()


def _state(fallback=0, mlp=False, min_len=2048):
    def put(e):
        e.set_fallback(fallback)
        if e.precision == "fp16c":
            e.set_mlp_compensation(mlp)
            e.set_f16c_min_len(min_len)
    return put


@pytest.mark.parametrize("prec", ["fp16c", "fp16x3", "fp16"])
def test_hyena_switch_history(hy, prec):
    """One handle, draw A, walked through its switches with a self-check on a padded batch between every two steps: at every step
    the probes equal a fresh handle put directly into that state, and with all switches back they equal the very first run."""
    if prec == "fp16c":
        walk = [("set_fallback(1)", dict(fallback=1)), ("set_fallback(2)", dict(fallback=2)), ("set_fallback(0)", dict()),
                ("set_mlp_compensation(True)", dict(mlp=True)), ("set_mlp_compensation(False)", dict()),
                ("set_f16c_min_len(1)", dict(min_len=1)), ("set_f16c_min_len(4098)", dict(min_len=4098)),
                ("set_f16c_min_len(2048)", dict())]
    else:
        walk = [("set_fallback(1)", dict(fallback=1)), ("set_fallback(0)", dict())]
    e = _maker(prec)()
    e.load_state_dict(hy["A"])
    probes = hy["probes"]

    def fresh_state(**kw):
        """The [PAD] tables stay over a switch (they are per arithmetic), and their values depend on the length class they were built
        for.  With the length switch at 4,098 the 3,000-token padded probe is the first padded batch an untouched fp16c handle runs in
        its fp16x3 kernels (table class 4,097), while the walked handle holds that table from its level-1 step (class 32,769): so a
        fresh fp16c handle first sees the long padded probe at level 1, as the walked one did, and is put into the state after it."""
        def put(h):
            if prec == "fp16c":
                h.set_fallback(1)
                h.forward(probes[0])
            _state(**kw)(h)
        return put

    try:
        first = before = _run(e, probes)
        assert_same_as_fresh(_maker(prec), hy["A"], None, probes, first, f"hyena {prec} untouched")
        _hy_anchor(hy, first, hy["A"], "A", H_TOL[prec], f"hyena {prec} switch walk, first run")
        for n, (name, kw) in enumerate(walk):
            _state(**kw)(e)
            after = _run(e, probes)
            assert_same_as_fresh(_maker(prec), hy["A"], fresh_state(**kw), probes, after, f"hyena {prec} {name}")
            d = _maxdiff(before, after)
            print(f"hyena {prec} switch {name}: max |before - after| {max(d):.2e}, == fresh")
            assert not _same(before, after), f"hyena {prec} {name}: the switch changed no probe"
            diff, _ = e.selfcheck(hy["warm"][n % 2])                         # the referee pass builds tables / filters of its own
            assert np.isfinite(diff) and diff <= 10 * H_TOL[prec]
            assert _same(after, _run(e, probes)), f"hyena {prec} {name}: the self-check changed the mode's bits"
            before = after
        assert _same(first, before), f"hyena {prec}: all switches back, but not the first run's bits"
    finally:
        e.close()


def _big(value):                                                # tests/test_gpu_parity.py::_big_weight_sd
    sdw = ho.make_state_dict(0, head_scale=3.0)
    sdw[BB + "layers.1.mixer.in_proj.weight"][5, 17] = value
    return sdw


@pytest.mark.parametrize("prec,level", [("fp16x3", 0), ("fp16c", 1)])
def test_hyena_range_verdict_unsticks_both_ways(hy, prec, level):
    """|w| = 300 pushes what would run fp16x3 to exact fp32; the plain draw loaded into the SAME handle brings fp16x3 back, and the
    reverse order pushes it out again.  A NaN weight (`x3_wmax` holds NaN by design) must not survive the reload either."""
    put = _state(fallback=level) if level else None
    plain, big, nan = hy["A"], _big(300.0), _big(float("nan"))
    probes = hy["probes"]
    e = _maker(prec)()
    try:
        want = None
        for n, (name, sd, arith) in enumerate((("|w| = 300", big, "fp32"), ("plain", plain, "fp16x3"), ("|w| = 300 again", big, "fp32"),
                                               ("plain again", plain, "fp16x3"), ("NaN", nan, "fp32"), ("plain after NaN", plain, "fp16x3"))):
            e.load_state_dict(sd)
            if put:
                put(e)
            assert e.effective_precision(1000) == arith, f"hyena {prec} level {level}, {name}: runs {e.effective_precision(1000)}"
            if sd is nan:
                continue                                         # (nothing to compare: every logit is NaN)
            got = _run(e, probes)
            fresh = assert_same_as_fresh(_maker(prec), sd, put, probes, got, f"hyena {prec} level {level}: {name}")
            if sd is plain:
                _hy_anchor(hy, got, plain, "A", H_TOL["fp16x3"], f"hyena {prec} level {level}: {name}")
                if want is not None:
                    assert _same(want, got)
                want = got
            else:
                before = fresh
            if sd is plain and n == 1:
                _moved(before, got, H_TOL["fp16x3"], f"hyena {prec} level {level}: |w| = 300 -> plain draw ({arith})", every=False)
            else:
                print(f"hyena {prec} level {level}: {name} runs {arith}, == fresh")
    finally:
        e.close()


def test_hyena_switches_are_handle_state_not_weight_state(hy):
    """At the ABI level the fall-back level, the MLP compensation and the short-read length stay over `clm_finalize`
    (include/chimeralm_hip.h says so; `HyenaDna.engine` resets them itself)."""
    probes = hy["probes"]
    e = _maker("fp16c")()
    try:
        e.load_state_dict(hy["A"])
        put = _state(fallback=1, mlp=True, min_len=1)
        put(e)
        for t in hy["warm"]:
            e.forward(t)
        e.load_state_dict(hy["B"])
        assert e.effective_precision(300) == "fp16x3" and e.effective_precision(20000) == "fp16x3"
        assert_same_as_fresh(_maker("fp16c"), hy["B"], put, probes, _run(e, probes), "hyena fp16c: level 1 kept over a reload")
        e.set_fallback(0)                                        # what is left: hi + lo MLP weights at every length
        assert e.effective_precision(300) == "fp16c"
        got = _run(e, probes)
        assert_same_as_fresh(_maker("fp16c"), hy["B"], _min1_mlp, probes, got, "hyena fp16c: mlp_lo and min_len kept over a reload")
        _hy_anchor(hy, got, hy["B"], "B", H_TOL["fp16c"], "hyena fp16c: switches kept over a reload")
        for name, other in (("mlp_lo", _min1), ("min_len", lambda h: h.set_mlp_compensation(True))):
            fresh = _maker("fp16c")()
            fresh.load_state_dict(hy["B"])
            other(fresh)
            differs = not _same(got, _run(fresh, probes))
            fresh.close()
            assert differs, f"{name} makes no difference on these probes: the scenario is vacuous"
        print("hyena fp16c: fall-back level, mlp_lo, f16c_min_len kept over clm_finalize, == fresh")
    finally:
        e.close()


def test_hyena_a_refused_load_changes_nothing(hy):
    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import EngineError

    probes = hy["probes"][1:4]
    e = _maker("fp16c")()
    try:
        e.load_state_dict(hy["A"])
        before = _run(e, probes)
        with pytest.raises(EngineError, match="does not match") as ei:
            e.load_weight(HD + "output_layer.bias", torch.zeros(3))
        assert ei.value.code == N.E_INVALID
        with pytest.raises(EngineError, match="unknown weight key"):
            e.load_weight(HD + "output_layer.gain", torch.zeros(2))
        with pytest.raises(EngineError, match="unknown weight key"):
            e.load_weight("net.tail.weight", torch.zeros(2))
        assert _same(before, _run(e, probes)), "a refused load changed the next forward"       # (no finalize in between)
        e.load_weight(HD + "output_layer.bias", hy["A"][HD + "output_layer.bias"])
        for call in (lambda: e.forward(probes[0]), lambda: e.selfcheck(probes[0]), lambda: e.reserve(2, 300), lambda: e.set_fallback(1)):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == N.E_STATE
        e.finalize()
        assert _same(before, _run(e, probes))
        print("hyena fp16c: refused loads change nothing; a loaded weight blocks forward / selfcheck / reserve / set_fallback until finalize")
    finally:
        e.close()


# ================================================================================================ 2. transformer
_TF_SHAPES = ((4, 4096, 0), (3, 777, 40), (16, 512, 0))


def _tf_make(prec, selfcheck=False):
    def make():
        from chimeralm_amd.transformer import SequenceCNNTransformer

        return SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=12, precision=prec, selfcheck=selfcheck)
    return make


@pytest.fixture(scope="module")
def tf(built_lib):
    warm = [torch.from_numpy(to.synthetic_ids(40 + i, *s)).cuda() for i, s in enumerate(_TF_SHAPES)]
    probe_np = [to.synthetic_ids(50 + i, *s) for i, s in enumerate(_TF_SHAPES)]
    return {"warm": warm, "probe_np": probe_np, "probes": [torch.from_numpy(x).cuda() for x in probe_np],
            "A": to.make_state_dict(0, to.PRODUCTION, scale=3.0), "B": to.make_state_dict(5, to.PRODUCTION, scale=1.0)}


def _tf_anchor(tf, got, sd, bound, what, name=None):
    """The probes against the oracle on `sd` (cached under `name`: the modes share their state dicts)."""
    if name is None or ("tf", name) not in _ORACLE:
        _ORACLE[("tf", name)] = [to.forward(torch.from_numpy(x), sd).numpy() for x in tf["probe_np"]]
    err = max(_maxdiff(got, _ORACLE[("tf", name)]))
    print(f"{what}: |logits - oracle| {err:.2e} (bound {bound:.1e})")
    assert err < bound, f"{what}: |logits - oracle| {err:.2e} > {bound}"


def _tf_warmed(tf, prec, sd=None):
    net = _tf_make(prec)()
    net.load_state_dict(tf["A"] if sd is None else sd)
    for t in tf["warm"]:
        net(t)
    return net, _run(net, tf["probes"])


@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16c", "fp16", "bf16"])
def test_transformer_full_reload(tf, prec):
    """Draw 0 at scale 3, the warm-up, then draw 5 at scale 1 into the same handle.  bf16's bound is 0.4 and the two draws' logits
    are only 2.0 .. 3.6 apart (oracle), under 10x that: its FIRST draw is stretched to scale 6 (9.5 .. 16.3 apart) instead."""
    net, before = _tf_warmed(tf, prec, to.make_state_dict(0, to.PRODUCTION, scale=6.0) if prec == "bf16" else None)
    try:
        net.load_state_dict(tf["B"])
        after = _run(net, tf["probes"])
        assert_same_as_fresh(_tf_make(prec), tf["B"], None, tf["probes"], after, f"transformer {prec} A -> B")
        _moved(before, after, TF_TOL[prec], f"transformer {prec}: full reload, draw 0 x 3 -> draw 5 x 1")
        _tf_anchor(tf, after, tf["B"], TF_TOL[prec], f"transformer {prec} after the reload", name="B")
    finally:
        net.close()


_TF_EDITS = [("cnn.3.weight", -1.0), ("transformer_encoder.layers.3.linear1.weight", -1.0),
             ("transformer_encoder.layers.0.self_attn.in_proj_weight", -1.0), ("attn_pool.weight", -4.0),
             ("transformer_encoder.layers.11.norm2.bias", -8.0), ("classifier.3.weight", -1.0)]


@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16c"])
def test_transformer_one_key_at_a_time(tf, prec):
    """In-place edits through the module (`with torch.no_grad(): p.mul_()`), cumulative: each reloads the one handle in place.
    `attn_pool.weight` does not show in the logits of seeded weights (after twelve layers the positions of a read are alike to
    ~1e-6, so how they are weighted does not matter: the oracle's logits move by 5e-6 for a factor of -4), so the pooling scores of
    the last probe (`debug_fetch("scores")`) are compared with the fresh handle's as well, and they are what must move for that key."""
    def run(m, probes):
        out = _run(m, probes)
        return out + [m.debug_fetch("scores", (probes[-1].shape[0], probes[-1].shape[1] // 8))]

    net, _ = _tf_warmed(tf, prec)
    before = run(net, tf["probes"])
    try:
        for key, factor in _TF_EDITS:
            h = net._h
            with torch.no_grad():
                _tensor(net, key).mul_(factor)
            after = run(net, tf["probes"])
            assert net._h is h                                   # the SAME handle, reloaded
            sd = _clone(net.state_dict())
            what = f"transformer {prec}: {key} x {factor:g}"
            assert_same_as_fresh(_tf_make(prec), sd, None, tf["probes"], after, what, run=run)
            if key == "attn_pool.weight":
                _moved(before[-1:], after[-1:], TF_TOL[prec], what + " (pooling scores)")
            else:
                _moved(before[:-1], after[:-1], TF_TOL[prec], what)
            _tf_anchor(tf, after[:-1], sd, TF_TOL[prec], what, name=what.split(": ")[1])
            before = after
    finally:
        net.close()


@pytest.mark.parametrize("prec", ["fp16c", "fp16x3"])
def test_transformer_fallback_walk(tf, prec):
    """`clm_tf_set_fallback` 1 / 2 / 0 with `clm_tf_selfcheck` in between on a warmed handle: every state equals a fresh handle put
    into it, and level 0 again gives the first run's bits."""
    from chimeralm_amd import _native as N

    lib = N.load()
    net, first = _tf_warmed(tf, prec)

    def level(n):
        def put(m):
            m(tf["probes"][1])                                   # (the module creates its handle at the first forward)
            assert lib.clm_tf_set_fallback(m._h, n) == 0
        return put

    try:
        before = first
        for n in (1, 2, 0):
            assert lib.clm_tf_set_fallback(net._h, n) == 0
            after = _run(net, tf["probes"])
            assert_same_as_fresh(_tf_make(prec), tf["A"], level(n), tf["probes"], after, f"transformer {prec} level {n}")
            d = _maxdiff(before, after)
            print(f"transformer {prec} clm_tf_set_fallback({n}): max |before - after| {max(d):.2e}, == fresh")
            if not (prec == "fp16x3" and n == 2):                # (an fp16x3 handle: levels 1 and 2 are both exact fp32)
                assert not _same(before, after)
            d_check = net._measure(lib, "history", tf["warm"][1])
            assert 0 < d_check <= TF_TOL[prec]
            assert _same(after, _run(net, tf["probes"]))
            before = after
        assert _same(first, before)
        _tf_anchor(tf, before, tf["A"], TF_TOL[prec], f"transformer {prec} fallback walk, level 0 again", name="A")
    finally:
        net.close()


def test_transformer_range_verdict_both_ways(tf):
    """One CNN-stem weight at 300 in place: `precision_report["fallback"]` True, then (the value put back) False, then True again;
    the bits are a fresh module's each time."""
    net, before = _tf_warmed(tf, "fp16x3")
    w = net.cnn[3].weight
    old = float(w.detach().view(-1)[1234])
    try:
        for value, fallback in ((300.0, True), (old, False), (300.0, True)):
            with torch.no_grad():
                w.view(-1)[1234] = value
            after = _run(net, tf["probes"])
            rep = net.precision_report
            assert rep["fallback"] is fallback and rep.get("fallback_precision") == ("fp32" if fallback else None), rep
            sd = _clone(net.state_dict())
            fresh_net = []

            def make():
                fresh_net.append(_tf_make("fp16x3")())
                return fresh_net[0]

            what = f"transformer fp16x3: cnn.3.weight[1234] = {value:g} (fallback {fallback})"
            assert_same_as_fresh(make, sd, None, tf["probes"], after, what)
            assert fresh_net[0].precision_report["fallback"] is fallback
            _moved(before, after, TF_TOL["fp16x3"], what, every=False)
            _tf_anchor(tf, after, sd, TF_TOL["fp16x3"], what)
            before = after
    finally:
        net.close()


class _TfHandle:
    """`clm_tf_*` through ctypes, for what the module does not do: a `pos_encoder.pe` of another length into the same handle."""

    def __init__(self, prec):
        from chimeralm_amd import _native as N

        self.N, self.lib, self.h = N, N.load(), C.c_void_p()
        assert self.lib.clm_tf_create(0, N.PRECISIONS[prec], 12, C.byref(self.h)) == 0

    def load_state_dict(self, sd):
        for k, t in sd.items():
            t = t.detach().float().contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            rc = self.lib.clm_tf_load_weight(self.h, k.encode(), C.c_void_p(t.data_ptr()), self.N.DT_F32, shape, t.dim())
            assert rc == 0, self.lib.clm_tf_last_error(self.h).decode()
        assert self.lib.clm_tf_finalize(self.h) == 0, self.lib.clm_tf_last_error(self.h).decode()

    def forward_rc(self, ids):
        out = torch.empty((ids.shape[0], 2), dtype=torch.float32, device=ids.device)
        rc = self.lib.clm_tf_forward(self.h, C.c_void_p(ids.data_ptr()), self.N.DT_I64, ids.stride(0), ids.shape[0], ids.shape[1],
                                     C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(ids.device).cuda_stream))
        return rc, out

    def __call__(self, ids):
        rc, out = self.forward_rc(ids)
        assert rc == 0, self.lib.clm_tf_last_error(self.h).decode()
        return out

    def close(self):
        if self.h:
            self.lib.clm_tf_destroy(self.h)
            self.h = None


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_transformer_pos_encoder_of_another_length(tf, prec):
    """Through the C ABI: `pos_encoder.pe` with 64 rows, then with 4,096 rows into the same handle.  A 1,000-token batch (125
    positions) is refused before and equals a fresh handle's after."""
    pe = tf["A"]["pos_encoder.pe"]
    short_sd, long_sd = {**tf["A"], "pos_encoder.pe": pe[:, :64].contiguous()}, {**tf["A"], "pos_encoder.pe": pe[:, :4096].contiguous()}
    small = torch.from_numpy(to.synthetic_ids(60, 3, 400)).cuda()
    ids_np = [to.synthetic_ids(61, 3, 1000), to.synthetic_ids(62, 2, 400, 30)]
    probes = [torch.from_numpy(x).cuda() for x in ids_np]
    h = _TfHandle(prec)
    try:
        h.load_state_dict(short_sd)
        before = h(small).cpu().numpy()
        rc, _ = h.forward_rc(probes[0])
        assert rc != 0 and "Sequence too long" in h.lib.clm_tf_last_error(h.h).decode()
        h.load_state_dict({"pos_encoder.pe": long_sd["pos_encoder.pe"]})       # ONE key, then finalize
        got = _run(h, probes)
        assert_same_as_fresh(lambda: _TfHandle(prec), long_sd, None, probes, got, f"transformer {prec}: pos_encoder.pe 64 -> 4,096 rows")
        assert np.array_equal(before, h(small).cpu().numpy())                  # the rows both tables share: the same bits
        err = max(_maxdiff(got, [to.forward(torch.from_numpy(x), tf["A"]).numpy() for x in ids_np]))
        print(f"transformer {prec}: pos_encoder.pe 64 -> 4,096 rows, 3 x 1,000 refused before, |logits - oracle| {err:.2e} after, == fresh")
        assert err < TF_TOL[prec]
    finally:
        h.close()


def test_transformer_guarded_module_after_a_fallback(tf):
    """fp16c with its guard at scale 3 falls back to fp16x3; `load_state_dict` of a draw at scale 0.25 puts the mode on trial again:
    the report is empty of a fall-back, the mode is kept, and the bits are a fresh guarded module's on the same batch sequence."""
    net = _tf_make("fp16c", selfcheck=True)()
    try:
        net.load_state_dict(tf["A"])
        with pytest.warns(RuntimeWarning, match="falling back to fp16x3"):
            before = _run(net, tf["probes"])
        assert net.selfcheck_report["fallback"] is True
        sd = to.make_state_dict(0, to.PRODUCTION, scale=0.25)
        net.load_state_dict(sd)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            after = _run(net, tf["probes"])
            fresh = []

            def make():
                fresh.append(_tf_make("fp16c", selfcheck=True)())
                return fresh[0]

            assert_same_as_fresh(make, sd, None, tf["probes"], after, "transformer guarded fp16c after a fall-back")
        rep = net.selfcheck_report
        assert rep["fallback"] is False and rep["precision"] == "fp16c" and rep["max_abs_dlogit"] <= rep["tol"]
        assert fresh[0].selfcheck_report == rep
        _moved(before, after, TF_TOL["fp16c"], "transformer guarded fp16c: scale 3 (fell back) -> scale 0.25 (kept)")
        _tf_anchor(tf, after, sd, TF_TOL["fp16c"], "transformer guarded fp16c at scale 0.25")
    finally:
        net.close()


# ================================================================================================ 3. CNN
def _cnn_make(prec):
    def make():
        from chimeralm_amd.cnn import DNAConvNet

        return DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                          hidden_dim=512, number_of_classes=2, dropout=0.1, precision=prec)
    return make


@pytest.fixture(scope="module")
def cnn(built_lib):
    probe_np = [cr.synthetic_ids(3100, 4, 8193, pads=100), cr.synthetic_ids(3101, 2, 777, pads=40)]
    return {"warm": [torch.from_numpy(cr.synthetic_ids(3000, 4, 8193)).cuda(), torch.from_numpy(cr.synthetic_ids(3001, 2, 777, pads=33)).cuda()],
            "probe_np": probe_np, "probes": [torch.from_numpy(x).cuda() for x in probe_np],
            "A": cr.make_cnn_state_dict(5), "B": cr.make_cnn_state_dict(6)}


def _cnn_anchor(cnn, got, sd, what, name=None):
    if name is None or ("cnn", name) not in _ORACLE:
        _ORACLE[("cnn", name)] = [cr.cnn_forward_fp64(sd, x).numpy() for x in cnn["probe_np"]]
    refs = _ORACLE[("cnn", name)]
    scale = max(1.0, max(float(np.abs(r).max()) for r in refs))               # (as tests/test_gpu_cnn.py does at |w| = 100)
    err = max(_maxdiff(got, refs))
    print(f"{what}: |logits - fp64| {err:.2e} (bound {CNN_TOL * scale:.1e})")
    assert err < CNN_TOL * scale
    return scale


def _cnn_warmed(cnn, prec):
    net = _cnn_make(prec)()
    net.load_state_dict(cnn["A"])
    for t in cnn["warm"]:
        net(t)
    return net, _run(net, cnn["probes"])


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_cnn_reload_and_one_key_at_a_time(cnn, prec):
    net, before = _cnn_warmed(cnn, prec)
    try:
        h = net._h.value
        net.load_state_dict(cnn["B"])
        after = _run(net, cnn["probes"])
        assert net._h.value == h                                 # reloaded in place
        assert_same_as_fresh(_cnn_make(prec), cnn["B"], None, cnn["probes"], after, f"cnn {prec} draw 5 -> 6")
        _moved(before, after, CNN_TOL, f"cnn {prec}: full reload, draw 5 -> draw 6")
        _cnn_anchor(cnn, after, cnn["B"], f"cnn {prec} after the reload", name="B")
        before = after
        for key, edit in (("embedding.weight", lambda w: w.mul_(-1.0)), ("conv_blocks.0.0.weight", lambda w: w.mul_(-0.5)),
                          ("conv_blocks.2.0.weight", lambda w: w.mul_(-1.0)), ("conv_blocks.1.1.running_mean", lambda w: w.add_(1.0)),
                          ("fc.1.weight", lambda w: w.mul_(-1.0)), ("fc.0.weight", lambda w: w.mul_(-1.0))):
            with torch.no_grad():
                edit(_tensor(net, key))
            after = _run(net, cnn["probes"])
            assert net._h.value == h
            sd = _clone(net.state_dict())
            what = f"cnn {prec}: {key}"
            assert_same_as_fresh(_cnn_make(prec), sd, None, cnn["probes"], after, what)
            _moved(before, after, CNN_TOL, what)
            _cnn_anchor(cnn, after, sd, what, name=key)
            before = after
    finally:
        net.close()


@pytest.mark.parametrize("key,index", [("conv_blocks.1.0.weight", (3, 17, 2)), ("fc.4.weight", (1, 200))])
def test_cnn_range_verdict_both_ways(cnn, key, index):
    """|w| = 100 in place and back.  `conv_blocks.1.0.weight`: the module recreates the handle as fp32 and back.  `fc.4.weight`: the
    module says fp32 where the engine's own `x3_active` (blocks 1 and 2 only) would not -- report and bits are the fp32 handle's."""
    net, before = _cnn_warmed(cnn, "fp16x3")
    first = before
    w = _tensor(net, key)
    old = float(w.detach()[index])
    try:
        for value, fallback in ((100.0, True), (old, False), (100.0, True), (old, False)):
            with torch.no_grad():
                w[index] = value
            after = _run(net, cnn["probes"])
            rep = net.precision_report
            assert rep["fallback"] is fallback and net._hprec == ("fp32" if fallback else "fp16x3"), rep
            sd = _clone(net.state_dict())
            what = f"cnn fp16x3: {key}{list(index)} = {value:g} (fallback {fallback})"
            assert_same_as_fresh(_cnn_make("fp16x3"), sd, None, cnn["probes"], after, what)
            if fallback:                                         # ... and an fp32 module's
                assert_same_as_fresh(_cnn_make("fp32"), sd, None, cnn["probes"], after, what + " vs an fp32 module")
            else:
                assert _same(first, after)
            scale = _cnn_anchor(cnn, after, sd, what, name=f"{key} = {value:g}")
            d = _maxdiff(before, after)
            print(f"{what}: max |before - after| {max(d):.2e}, == fresh")
            assert max(d) > 10 * CNN_TOL * scale, d              # (scale: 1 unless the logits themselves are large)
            before = after
    finally:
        net.close()


# ================================================================================================ 4. Mamba
def test_mamba_rerun_handle_follows_the_weights(built_lib):
    """`mambasp`, two layers, fp16x3, the embedding x 2^17: the batch is rerun on the exact-fp32 handle (`_h32`).  An in-place change
    of `A_log` that keeps the overflow: still rerun, and the logits are a fresh module's (the rerun handle does not keep the old
    weights).  The embedding scaled back in place: no rerun, a fresh fp16x3 module's bits.
    OPEN FINDING, not covered here: with `A_log + 0.7` instead, at this embedding scale, the exact-fp32 rerun itself returned NaN
    logits for two of the three 1,100-token reads (the fp64 forward is finite there), and the module hands them on."""
    from chimeralm_amd import mamba

    def make():
        return mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=512, number_of_layers=2, number_of_classes=2, dropout=0.2,
                                                   d_state=mr.VARIANTS["mambasp"][2], expand=mr.VARIANTS["mambasp"][3], precision="fp16x3")

    sd = mr.make_mamba_state_dict("mambasp", 26, n_layers=2)
    plain = _clone(sd)
    sd["embedding.weight"] = sd["embedding.weight"] * 131072.0
    ids_np = [mr.synthetic_ids(2600, 2, 300), mr.synthetic_ids(2601, 3, 1100, pads=50)]
    probes = [torch.from_numpy(x).cuda() for x in ids_np]

    def anchor(got, sd_now, what):
        refs = [mr.mamba_forward_fp64("mambasp", sd_now, x, device="cuda").cpu().numpy() for x in ids_np]
        scale = max(1.0, max(float(np.abs(r).max()) for r in refs))           # (relative, as tests/test_gpu_mamba.py at this scale)
        err = max(_maxdiff(got, refs))
        print(f"{what}: |logits - fp64| {err:.2e} (bound {MAMBA_TOL * scale:.1e})")
        assert err < MAMBA_TOL * scale
        return scale

    net = make()
    assert net._shape[0] == mr.VARIANTS["mambasp"][0]
    try:
        net.load_state_dict(sd)
        before = _run(net, probes)
        assert net.precision_report["nonfinite_reruns"] == 2 and all(np.isfinite(x).all() for x in before)
        with torch.no_grad():
            net.mamba_layers[1].A_log.sub_(0.7)
            # (at this scale dt saturates and the decay is exactly 0 whatever A is -- the fp64 forward's logits do not move at all
            # with A_log -- so a second tensor makes the event one that shows: the rerun handle holds every weight)
            net.classifier[0].weight.mul_(-1.0)
        after = _run(net, probes)
        assert all(np.isfinite(x).all() for x in after)
        assert net.precision_report["nonfinite_reruns"] == 2     # (counted per weight load: both probes of the new weights)
        net(probes[0])
        assert net.precision_report["nonfinite_reruns"] == 3     # ... and counting on
        sd2 = _clone(net.state_dict())
        assert_same_as_fresh(make, sd2, None, probes, after, "mambasp fp16x3 rerun on fp32: A_log - 0.7, classifier.0.weight x -1")
        scale = anchor(after, sd2, "mambasp fp16x3 rerun on fp32: A_log - 0.7, classifier.0.weight x -1")
        d = _maxdiff(before, after)
        print(f"mambasp fp16x3 rerun on fp32: A_log - 0.7, classifier.0.weight x -1: max |before - after| {max(d):.2e}, == fresh")
        assert min(d) > 10 * MAMBA_TOL * scale
        with torch.no_grad():
            net.embedding.weight.mul_(1.0 / 131072.0)            # (a power of two: the plain draw's embedding again, exactly)
        back = _run(net, probes)
        assert "nonfinite_reruns" not in net.precision_report and net._hprec == "fp16x3"
        plain["mamba_layers.1.A_log"], plain["classifier.0.weight"] = sd2["mamba_layers.1.A_log"], sd2["classifier.0.weight"]
        assert all(torch.equal(net.state_dict()[k], plain[k]) for k in plain)
        assert_same_as_fresh(make, plain, None, probes, back, "mambasp fp16x3: the embedding scaled back")
        anchor(back, plain, "mambasp fp16x3: the embedding scaled back")
        d = _maxdiff(after, back)
        print(f"mambasp fp16x3: the embedding scaled back: max |before - after| {max(d):.2e}, == fresh")
        assert min(d) > 10 * MAMBA_TOL
    finally:
        net.close()


# ================================================================================================ 5. edits through `.data`
def test_data_edit_needs_refresh_weights_hyena(hy):
    """`p.data.mul_()` does not move the reload signature (torch does not count it): the forward after it is STALE -- asserted, so
    that the limit stays visible -- until `refresh_weights()`; then it is a fresh module's, bit for bit."""
    from chimeralm_amd import lm

    def make():
        # (unguarded: a guard that moves its switches between two runs of the probes would hide what is asserted here)
        return lm.ChimeraLM.new(precision="fp16c", chunk_reads=4, selfcheck=False)

    # 4 x 20,000 padded, 3 x 3,000 padded, 2 x 6,000: all in the 16-bit kernels.  The longest first: the [PAD] table is then built for
    # its final length class by the first forward, and a second run of the probes on the same handle reads the same table (with the
    # 3,000-token batch first, the 6,000-token one regrew the table and the rerun differed by 1e-5 -- the carve-out above)
    probes = [hy["probes"][0], hy["probes"][1], hy["probes"][4]]
    m = make()
    try:
        m.load_state_dict(hy["A"], strict=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            before = _run(m.net, probes)
            assert _same(before, _run(m.net, probes))            # (the probes are repeatable on this handle: what follows is the edit)
            m.net.backbone.backbone.layers[0].mixer.filter_fn.implicit_filter[6].weight.data.mul_(-1.0)
            assert _same(before, _run(m.net, probes)), "an edit through .data was picked up: the documented limit moved"
            m.net.refresh_weights()
            after = _run(m.net, probes)
            sd = _clone(m.state_dict())

            class Fresh:                                         # (ClassificationLit: the net is what runs)
                def __init__(self):
                    self.m = make()

                def load_state_dict(self, s):
                    self.m.load_state_dict(s, strict=True)

                def __call__(self, t):
                    return self.m.net(t)

                def close(self):
                    self.m.net._engine.close()

            assert_same_as_fresh(Fresh, sd, None, probes, after, "HyenaDna fp16c: .data edit + refresh_weights()")
        _moved(before, after, H_TOL["fp16c"], "HyenaDna fp16c: implicit_filter.6.weight.data.mul_(-1) + refresh_weights()")
        refs = [ho.forward(torch.from_numpy(hy["probe_np"][1].astype(np.int64)), sd).numpy()]
        assert max(_maxdiff(after[1:2], refs)) <= H_TOL["fp16c"]
    finally:
        m.net._engine.close()


def test_data_edit_needs_refresh_weights_cnn(cnn):
    net, before = _cnn_warmed(cnn, "fp16x3")
    try:
        net.conv_blocks[1][0].weight.data.mul_(-1.0)
        assert _same(before, _run(net, cnn["probes"])), "an edit through .data was picked up: the documented limit moved"
        net.refresh_weights()
        after = _run(net, cnn["probes"])
        sd = _clone(net.state_dict())
        assert_same_as_fresh(_cnn_make("fp16x3"), sd, None, cnn["probes"], after, "DNAConvNet: .data edit + refresh_weights()")
        _moved(before, after, CNN_TOL, "DNAConvNet fp16x3: conv_blocks.1.0.weight.data.mul_(-1) + refresh_weights()")
        _cnn_anchor(cnn, after, sd, "DNAConvNet after refresh_weights()")
    finally:
        net.close()
