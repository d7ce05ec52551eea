"""Host (no GPU): tests/cnn_stage_reference.py against tests/cnn_reference.py and the golden file, the geometry the GPU shapes claim,
the float32 yardstick in every shape and regime, and the statistic of tests/test_gpu_cnn_stages.py against planted defects.

The planted defects are wrong REFERENCES, written here on the CPU, of the kinds a DNAConvNet kernel can have: a right halo that reads
zero where the read goes on, or the last row where the read has ended, or the neighbouring read's rows; one tap of seven without its
fp16x3 activation lo half; a ragged partial summed over a whole tile.  For each, at three of the GPU shapes, the per-position
statistic exceeds 16 x the float32 yardstick at exactly the positions the defect reaches and nowhere else -- at a shape the defect
cannot reach, nowhere at all, which is why the GPU cases are chosen by what they reach.  Next to it the test prints what the two gates
of tests/test_gpu_cnn.py see of the same defect (the logits against 1e-4; block0 / block1 / pooled against 1e-5 of the tensor's
maximum): whichever defects those pass, the statistic does not."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cnn_reference as cr
import cnn_stage_reference as S
import error_model as em

TOL, TOL_REL = 1e-4, 1e-5       # tests/test_gpu_cnn.py: logits (absolute), intermediates (of the tensor's maximum)
K = 16                          # the cap of tests/test_gpu_cnn_stages.py


# ------------------------------------------------------------------------------------------------------------- the chain
def test_the_chained_stages_are_the_reference_forward():
    sd = cr.make_cnn_state_dict(61)
    for B, L in ((3, 1075), (2, 127), (1, 64)):
        ids = S.stage_ids(6100 + L, B, L)
        want_tr, got_tr = {}, {}
        want = cr.cnn_forward_fp64(sd, ids, trace=want_tr)
        got = S.forward(sd, ids, torch.float64, trace=got_tr)
        assert float((got - want).abs().max()) <= 1e-12
        for k, v in want_tr.items():
            assert got_tr[k].shape == v.shape and float((got_tr[k] - v).abs().max()) <= 1e-12, k
        assert got_tr["partial"].shape == (B, S.geometry(L)["tiles2"], 256)
        assert float((got_tr["partial"].sum(1) / (L // 64) - got_tr["block2"].mean(1)).abs().max()) <= 1e-12


def test_the_chained_stages_are_the_golden_file(golden_dir):
    golden = np.load(golden_dir / "cnn_golden.npz")
    names = sorted(k[:-5] for k in golden.files if k.endswith("_meta"))
    assert len(names) == 5
    for name in names:
        seed = int(golden[f"{name}_meta"][0])
        got = S.forward(cr.make_cnn_state_dict(seed), golden[f"{name}_ids"], torch.float64).numpy()
        assert np.abs(got - golden[f"{name}_logits"]).max() < 1e-5, name


def test_stage_ids_are_the_three_reads():
    ids = S.stage_ids(6000, 3, 1075)
    assert (ids[0, :-1] == 4).all() and ids[0, -1] != 4
    assert not (ids[1] == 4).any() and not (ids[1] == 11).any()
    assert (ids[2] == 4).sum() == 3 and (ids[2, :3] == 4).all() and (ids[2] == 11).sum() == 1
    assert S.stage_ids(6000, 1, 64).shape == (1, 64)


# ------------------------------------------------------------------------------------------------------------- geometry
def test_every_gpu_shape_reaches_what_its_comment_claims():
    assert sorted({L for _, L in S.SHAPES}) == sorted(S.GEOMETRY)
    for L, claim in S.GEOMETRY.items():
        g = S.geometry(L)
        print(L, g)
        for k, v in claim.items():
            assert g[k] == v, (L, k, g[k], v)
    assert (1, 64) in S.SHAPES and all(B == 3 for B, L in S.SHAPES if L != 64)
    # the table as a whole: every count of real right-halo rows in both MFMA blocks, whole and one-row last tiles, one and several
    # block-0 workgroups with an empty, a one-position and a full second half
    gs = [S.geometry(L) for L in S.GEOMETRY]
    assert {g["halo1"] for g in gs} == {0, 1, 3} and {g["halo2"] for g in gs} >= {0, 3}
    assert {g["trail0"] for g in gs} >= {0, 3} and {g["trail1"] for g in gs} == {0, 1, 3} and {g["trail2"] for g in gs} >= {0, 3}
    assert {1, 16} <= {g["last_out1"] for g in gs} and {1, 16} <= {g["last_rows2"] for g in gs}
    assert {0, 1, 64} <= {g["last_half0"] for g in gs} and {1, 2, 5} <= {g["wg0"] for g in gs}


# ------------------------------------------------------------------------------------------------------------- the yardstick
def _yardsticks(sd, ids):
    """{stage: per-position statistic of the float32 stage on the float64 chain's input of that stage}."""
    tr: dict = {}
    S.forward(sd, ids, torch.float64, trace=tr)
    w32, w64 = S.weights(sd, torch.float32), S.weights(sd, torch.float64)
    f = lambda k: tr[k].float()                                       # noqa: E731
    up = lambda k: tr[k].float().double()                             # noqa: E731  (the reference on the SAME float32 input)
    L64 = tr["block2"].shape[1]
    idt = torch.from_numpy(ids)
    b2 = S.block(w32, 2, f("block1"))
    pairs = {"block0": (S.block0(w32, idt), tr["block0"]),
             "block1": (S.block(w32, 1, f("block0")), S.block(w64, 1, up("block0"))),
             "block2": (b2, S.block(w64, 2, up("block1"))),
             "partial": (S.tile_sums(b2), S.tile_sums(S.block(w64, 2, up("block1")))),
             "pooled": (S.pooled_from(f("partial"), L64)[:, None], S.pooled_from(up("partial"), L64)[:, None]),
             "logits": (S.head(w32, f("pooled"))[:, None], S.head(w64, up("pooled"))[:, None])}
    st = {k: S.statistic(y, r) for k, (y, r) in pairs.items()}
    st["|dlogit|"] = (pairs["logits"][0].double() - pairs["logits"][1]).abs().amax(-1)
    return st, tr


CASES = [(f"shape-B{B}-L{L}", "unit", S.SEED_SHAPES, 6400 + L, B, L) for B, L in S.SHAPES] + \
        [(f"regime-{r}", r, S.SEED_REGIMES, 6000, *S.REGIME_SHAPE) for r in ("unit",) + S.REGIMES]


@pytest.mark.parametrize("tag,regime,wseed,iseed,B,L", CASES, ids=[c[0] for c in CASES])
def test_the_float32_yardstick_is_below_the_old_gate(tag, regime, wseed, iseed, B, L):
    """K x the yardstick is a tighter bound than the old 1e-5 only where the yardstick is well below it: every stage, every position.
    Measured: at most 5.4e-7 per position in every shape and regime but `deep`, whose rows have maxima of 0.16 - 0.45 under
    pre-activations of order 1: 4.9e-6 (block 1), 5.4e-6 (block 2), 3.7e-6 (partial).  The logits are two numbers per read, and their
    own maximum is small by chance on some reads (up to 5.9e-6 of it): they are printed that way and held as the old gate holds them,
    absolutely, to 1e-5 (a tenth of that gate; measured: at most 3.3e-6 on logits of magnitude up to 5)."""
    st, tr = _yardsticks(S.regime_state_dict(regime, wseed), S.stage_ids(iseed, B, L))
    print(f"YARDSTICK {tag:18s} " + "  ".join(f"{k} {float(v.max()):.2e}" for k, v in st.items()))
    for k, v in st.items():
        assert bool(torch.isfinite(v).all()), (tag, k)
        if k != "logits":
            assert float(v.max()) < TOL_REL, (tag, k, float(v.max()))
    if regime == "deep":
        assert float(tr["block2"].abs().amax(-1).median()) < 0.25        # GELU's dip: no row far above its minimum's depth
    if regime.startswith("act2^-"):
        k = int(regime[6:])
        assert float(tr["block0"].abs().max()) < 16 * 2.0 ** -k and 0.5 < float(tr["block1"].abs().amax(-1).median()) < 4


# ------------------------------------------------------------------------------------------------------------- planted defects
def _pad_trailing_zero(x):
    """(a) the rows past 4 Lout, which the pool drops, read as zero: a kernel that stages only the rows that feed a window."""
    x = x.clone()
    x[:, 4 * (x.shape[1] // 4):] = 0.0
    return S.zero_pad(x)


def _pad_clamped(x):
    """(b) behind the read's end the last row again, not zero."""
    xp = S.zero_pad(x)
    xp[:, -S.HALO:] = x[:, -1:]
    return xp


def _pad_neighbour(x):
    """(c) the halo rows of the flattened [B x Lin] rows: the neighbouring read's."""
    xp = S.zero_pad(x)
    xp[1:, :S.HALO] = x[:-1, -S.HALO:]
    xp[:-1, -S.HALO:] = x[1:, :S.HALO]
    return xp


def _lin_one_lo_dropped(tap):
    """(d) fp16x3's three products with the activation lo half of tap `tap` missing."""
    def lin(a, W):
        ah, al = em.x3_split(a)
        wh, wl = em.x3_split(W.double() * em.X3_WS)
        al = al.clone()
        al[..., tap * S.D:(tap + 1) * S.D] = 0.0
        return (ah @ (wh + wl).T + al @ wh.T) / em.X3_WS
    return lin


def _partial_whole_tile(w, x):
    """(e) every partial a sum over 16 pooled rows: behind the last row, the windows a tile computes over the rows there are."""
    Lin = x.shape[1]
    tiles = -(-(Lin // 4) // S.ROWS2)
    rows = S.block(w, 2, torch.nn.functional.pad(x, (0, 0, 0, max(0, tiles * S.TILE - Lin))))   # (zero rows behind the read, as staged)
    return S.tile_sums(rows[:, :tiles * S.ROWS2])


def _reached(x, pad):
    """The pooled positions [B, Lout] whose windows read a row that `pad` changes: window p covers padded rows 4 p .. 4 p + 9."""
    changed = (pad(x) != S.zero_pad(x)).any(-1)                      # [B, Lin + 6]
    Lout = x.shape[1] // 4
    return torch.stack([changed[:, 4 * p:4 * p + 4 + 2 * S.HALO].any(1) for p in range(Lout)], dim=1)


MUTANTS = ("a-trailing-rows-zero", "b-halo-clamped", "c-halo-from-neighbour", "d-one-lo-half-dropped", "e-partial-over-16")
MUTANT_SHAPES = (127, 1075, 1091)


@pytest.fixture(scope="module")
def chains():
    out = {}
    sd = cr.make_cnn_state_dict(S.SEED_REGIMES)
    for L in MUTANT_SHAPES:
        ids = S.stage_ids(6000, 3, L)
        tr: dict = {}
        logits = S.forward(sd, ids, torch.float64, trace=tr)
        out[L] = (sd, ids, tr, logits)
    return out


@pytest.mark.parametrize("L", MUTANT_SHAPES)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_planted_defect_is_named_where_it_reaches_and_nowhere_else(chains, mutant, L):
    sd, ids, tr, logits = chains[L]
    w64, w32 = S.weights(sd, torch.float64), S.weights(sd, torch.float32)
    idt = torch.from_numpy(ids)
    emb = w64["embedding.weight"][idt]
    # (stage, its input, the unplanted float64 stage, the float32 yardstick, the planted stage, the positions it reaches)
    todo = []
    if mutant[0] in "abc":
        pad = {"a": _pad_trailing_zero, "b": _pad_clamped, "c": _pad_neighbour}[mutant[0]]
        for i, k_in in ((0, None), (1, "block0"), (2, "block1")):
            x = emb if i == 0 else tr[k_in]
            todo.append((f"block{i}", S.block(w64, i, x), S.block(w32, i, x.float()), S.block(w64, i, x, pad=pad), _reached(x, pad),
                         lambda w, inp, i=i: S.block(w, i, inp if i else w["embedding.weight"][inp], pad=pad)))
    elif mutant[0] == "d":
        for i, k_in in ((1, "block0"), (2, "block1")):
            x = tr[k_in]
            wrong = S.block(w64, i, x, lin=_lin_one_lo_dropped(3))
            whole = S.block(w64, i, x, lin=em.x3_linear)
            assert float(S.statistic(whole, tr[f"block{i}"]).max()) < 2e-7   # the format itself: below the float32 yardstick
            todo.append((f"block{i}", S.block(w64, i, x), S.block(w32, i, x.float()), wrong, torch.ones(wrong.shape[:2], dtype=torch.bool),
                         lambda w, inp, i=i: S.block(w, i, inp, lin=_lin_one_lo_dropped(3))))
    else:
        x = tr["block1"]
        L64 = x.shape[1] // 4
        reached = torch.zeros(3, -(-L64 // S.ROWS2), dtype=torch.bool)
        reached[:, -1] = L64 % S.ROWS2 != 0
        todo.append(("partial", tr["partial"], S.tile_sums(S.block(w32, 2, x.float())), _partial_whole_tile(w64, x), reached, _partial_whole_tile))
    for stage, ref, yard, wrong, reached, replace in todo:
        e, y = S.statistic(wrong, ref), S.statistic(yard, ref)
        bound = torch.maximum(K * y.amax(1, keepdim=True), torch.tensor(S.FLOOR, dtype=torch.float64))
        flagged = e > bound
        # the gates of tests/test_gpu_cnn.py on the same defect: the logits, and the tensors it fetches, each over the tensor's maximum
        wtr: dict = {}
        wl = S.forward(sd, ids, torch.float64, trace=wtr, replace={stage: replace})
        d_logit = float((wl - logits).abs().max())
        gates = {k: float((wtr[k] - tr[k]).abs().max() / tr[k].abs().max()) for k in ("block0", "block1", "pooled")}
        old_pass = d_logit < TOL and all(v < TOL_REL for v in gates.values())
        rows, bad = [], []
        S.check(f"{mutant} L{L}", stage, e, y, K, rows, bad)
        print(f"MUTANT {mutant:24s} L {L:4d} {stage:8s} reaches {int(reached.sum()):4d} of {reached.numel():4d} positions; statistic: max "
              f"{float(e.max()):.2e} (yardstick {float(y.max()):.2e}), flags {int(flagged.sum()):4d}, {len(bad)} figures fail | old gates: "
              f"|dlogit| {d_logit:.2e} (1e-4), " + ", ".join(f"{k} {v:.2e}" for k, v in gates.items()) + f" (1e-5): {'PASS' if old_pass else 'fail'}")
        assert torch.equal(flagged, reached), (stage, flagged.nonzero().tolist()[:8], reached.nonzero().tolist()[:8])
        assert float(e[~reached].max() if (~reached).any() else 0.0) == 0.0 or mutant[0] == "d"
        assert bool(bad) == bool(reached.any())
        if reached.any():
            for b in range(3):
                if reached[b].any():
                    assert any(f"read {b} max" in line for line in bad), "\n".join(rows)
            assert not (old_pass and not bad)                        # whatever the old gates pass, the statistic does not


def test_the_unplanted_yardstick_passes_its_own_bound(chains):
    sd, ids, tr, _ = chains[1075]
    w32 = S.weights(sd, torch.float32)
    y = S.statistic(S.block(w32, 1, tr["block0"].float()), tr["block1"])
    rows, bad = [], []
    S.check("host", "block1", y, y, K, rows, bad)
    assert not bad
