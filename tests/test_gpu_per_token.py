"""GPU (MI355X): the Hyena engine's residual rows and pooling scores against the fp64 oracle, TOKEN BY TOKEN, on the production plan.

Almost every Hyena GPU test judges the kernels through the two logits -- an attention-weighted mean over the whole read pushed through a
small head, on which an error confined to one token of 8,193 (the aliased last output of an L = N/2 + 1 transform, the two patched
tokens of a tile range, the peeled [SEP], the first token of a segment, a pair partner leaking through the packed transform) stays
two orders below the gates (tests/test_per_token_host.py shows it).  Here every token is held to the oracle's float64 forward by
itself (tests/per_token_reference.py), after a FULL forward -- no debug stop, no CLM_DEBUG: the production plan.

WHAT IS COMPARED.  `debug_fetch("scores")`: the pooling score of every token, in every mode.  `debug_fetch("h")`: the residual rows
the forward leaves behind, and which rows those are follows from the code, not from the fetch:
  * fp32, fp16x3 (tail32.hip): the fused tail stores h' in every block (step 4), the last one included, and rows of tiles inside a
    [PAD] prefix are filled from the all-[PAD] table (pad_prefix.hip prefix_fill_h_kernel): block 3's rows, all of them, = l3.out.
  * fp16c, fp16, bf16 (gemm16.hip tail16_kernel): the LAST block's output is consumed on chip by the score / pooling stage and is
    NOT stored ("if constexpr (NEXT != NEXT_SCORE)" in front of the store of step 5; lone_token.hip "if (!a.last) a.h[...] ="; and
    clm_rows refuses 16-bit rows for the same reason).  So `h` holds BLOCK 2's rows (l2.out) -- written by the tile kernels and,
    for the peeled token, by lone_token.hip -- and those are what is compared, against the oracle's l2.out.  Block 3 of these modes
    is held per token through its scores: a token's score is a function of its block-3 row alone.
    With [PAD]-prefix skipping (clm_api.hip plan_chunk: pad_skip, L >= 256) the tile list of a read starts ONE tile before its first
    non-prefix tile (pad_prefix.hip tile_list_kernel: start = p0 - 1) and no 16-bit kernel ever writes the rows before it: they are
    left out through rows= (whole 128-token tiles of a prefix; read 0 of every batch, read 1 of the two long-prefix shapes).  No
    other row is left out in any mode, the peeled token's included.  The scores of every token are always compared (the prefix's
    come from the table, prefix_fill_pool_kernel).

SHAPES.  B = 3 (odd: one unit of the packed transform holds a single read); read 0 is all [PAD] up to its [SEP] (pair (0, 1): leakage
between partners), the others get 3 pads.  1, 2, 65: shorter than a tile.  129 ... 4097: L = N/2 + 1 of every one-shot transform
(256 ... 8192 points), the aliased last output; the lone peeled token of the 16-bit modes.  300, 1000, 3000: ragged last tiles.
4098, 6000, 8193: the persistent 16384-point kernel (first length, ragged unit, bench length).  8194: the first segmented length
(two tokens in segment 1).  16385: segmented with the dot-product tail.  20000: three segments, ragged.  1000 with 300 and 20000
with 9000 pads on read 1: prefix tile skipping and, in fp16c, prefix segment skipping.  fp32 and fp16x3 run everywhere; fp16c at
L >= 2049 and, its length switch moved down (set_f16c_min_len(1)), at 257, 513, 1000; fp16 and bf16 at 513, 2049, 8193, 16385.

BOUNDS.  Per read: max and rms over tokens of the per-token error <= K x the same statistic of a yardstick.
  * fp32, fp16x3: the yardstick is the reference's own arithmetic, the oracle's float32 forward.  K = 16: the smallest power of two
    >= 2 x the worst measured ratio (6.85), the cap the issue allows; fp16x3 claims fp32 class and gets the same K.
  * fp16c, fp16, bf16: the yardstick is the CPU error model (tests/error_model.py ENGINE_MODES: an fp64 forward rounding where the
    kernels round -- GEMM operands, packed weights, y, the gated rows of z behind the short filter, block 0 from the fp32 id table,
    the peeled token through unrounded products; fp16c: hi + e4m3 lo weights for in_proj / out_proj / attention.0, plain fp16 fc1 /
    fc2, e5m2 lo bytes for the LayerNorm-1 / ln_f tiles, y and z).  K16 = 4: the smallest power of two >= 2 x 1.95.  fp16 and bf16
    follow the model to 1-2 % in rms at every length; fp16c sits 1.3-1.95 x above it (the truncated hi bytes inside its two lo
    products are not modelled).
  * 16-bit modes, structure: tokens 0-1 of every 128-token tile, the last token and the first token of every 8192-token segment
    each stay within the line of all tokens; a failure names the class.

FINDING (first run, before any bound was set).  Exact fp32 and fp16x3 at 1 and 2 tokens: hidden 9.0-12.3 x and scores 8.2-25.5 x
the float32 oracle, above the 8 x that asks for an explanation.  The separate GEMM kernels (stage stops) measured 3.6e-7 of a
row's maximum at 2 tokens, the fused tail 2.4e-6 -- at every token of every length, which only the shortest reads show because the
oracle's own error is ten times smaller there (2e-7) than from 65 tokens on (2e-6).  Cause: tail32_kernel started its accumulators
from the residual row, so each of the 128 + 512 MFMA steps of out_proj and fc2 rounded at the residual's magnitude.  Fixed in
tail32.hip (sums from zero, the residual in registers of its own).  Before -> after, worst ratio: 1 token 9.52 -> 1.61 (scores 8.23
-> 2.10), 2 tokens 12.25 -> 1.73 (scores 25.9 -> 5.59); rms over tokens at every length from 65 on: 1.2-2.3 -> 0.43-1.65.

MEASURED on the MI355X, this tree: engine statistic / yardstick statistic, worst read of the batch.
      L  pads   hidden       scores       yardstick (worst token)
                max   rms    max   rms    hidden    scores
  fp32
         1     3    1.61  1.61    2.10  2.10    1.89e-07  8.56e-07
         2     3    1.73  1.67    4.81  5.59    2.05e-07  4.96e-07
        65     3    0.43  0.43    0.62  0.44    2.27e-06  7.86e-06
       129     3    0.60  0.44    0.87  0.56    2.14e-06  8.44e-06
       257     3    2.10  0.91    1.16  1.10    2.97e-06  1.10e-05
       513     3    2.47  0.75    1.83  1.06    2.72e-06  1.19e-05
      1025     3    2.24  0.68    1.20  0.76    3.07e-06  1.29e-05
      2049     3    1.65  0.61    1.22  0.65    8.23e-06  2.66e-05
      4097     3    2.00  0.65    1.90  0.77    1.27e-05  6.81e-05
       300     3    4.72  1.65    5.22  2.79    2.56e-06  9.35e-06
      1000     3    3.79  0.97    4.76  1.05    3.01e-06  1.02e-05
      3000     3    2.22  0.66    1.58  0.68    5.29e-06  3.69e-05
      4098     3    1.25  0.63    0.84  0.70    8.07e-06  5.52e-05
      6000     3    2.12  0.67    1.66  0.72    5.20e-06  3.40e-05
      8193     3    1.70  0.65    1.20  0.67    6.57e-06  4.03e-05
      8194     3    1.14  0.62    1.15  0.71    1.00e-05  3.37e-05
     16385     3    1.04  0.55    0.94  0.67    1.31e-05  7.71e-05
     20000     3    3.33  0.56    1.97  0.70    5.02e-06  3.38e-05
      1000   300    3.58  0.98    3.87  1.02    3.01e-06  1.08e-05
     20000  9000    1.94  0.56    1.91  0.70    5.72e-06  3.38e-05
  fp16x3
         1     3    0.78  0.78    0.76  0.76    1.89e-07  8.56e-07
         2     3    1.18  1.10    4.98  4.77    2.05e-07  4.96e-07
        65     3    0.46  0.36    0.50  0.34    2.27e-06  7.86e-06
       129     3    0.50  0.39    0.67  0.53    2.14e-06  8.44e-06
       257     3    1.92  0.92    1.09  1.15    2.97e-06  1.10e-05
       513     3    2.25  0.74    1.73  1.08    2.72e-06  1.19e-05
      1025     3    2.14  0.63    1.14  0.70    3.07e-06  1.29e-05
      2049     3    1.66  0.59    1.10  0.62    8.23e-06  2.66e-05
      4097     3    2.02  0.62    1.83  0.70    1.27e-05  6.81e-05
       300     3    4.77  1.61    6.09  2.74    2.56e-06  9.35e-06
      1000     3    3.83  0.95    5.55  1.03    3.01e-06  1.02e-05
      3000     3    2.07  0.63    1.57  0.64    5.29e-06  3.69e-05
      4098     3    1.27  0.61    0.89  0.69    8.07e-06  5.52e-05
      6000     3    2.07  0.64    1.80  0.84    5.20e-06  3.40e-05
      8193     3    1.92  0.59    1.20  0.75    6.57e-06  4.03e-05
      8194     3    1.29  0.58    1.83  0.81    1.00e-05  3.37e-05
     16385     3    1.07  0.49    1.02  0.70    1.31e-05  7.71e-05
     20000     3    3.54  0.50    2.26  0.82    5.02e-06  3.38e-05
      1000   300    4.06  1.05    6.85  1.62    3.01e-06  1.08e-05
     20000  9000    2.16  0.50    3.37  0.82    5.72e-06  3.38e-05
  fp16c
      2049     3    1.28  1.37    1.25  1.26    1.83e-04  1.08e-03
      4097     3    1.55  1.59    1.34  1.35    1.77e-04  1.08e-03
      3000     3    1.46  1.48    1.17  1.30    1.91e-04  1.08e-03
      4098     3    1.53  1.58    1.56  1.34    1.73e-04  1.08e-03
      6000     3    1.51  1.45    1.20  1.35    1.82e-04  1.08e-03
      8193     3    1.49  1.72    1.16  1.37    1.96e-04  1.08e-03
      8194     3    1.49  1.71    1.48  1.40    1.86e-04  1.08e-03
     16385     3    1.63  1.68    1.22  1.51    1.80e-04  1.08e-03
     20000     3    1.89  1.95    1.22  1.55    1.64e-04  1.08e-03
     20000  9000    1.89  1.95    1.22  1.55    1.64e-04  1.08e-03
  fp16c-forced
       257     3    1.05  1.08    1.21  1.02    2.08e-04  1.08e-03
       513     3    1.19  1.17    1.26  1.10    1.66e-04  1.08e-03
      1000     3    1.20  1.31    1.21  1.13    2.03e-04  1.08e-03
  fp16
       513     3    1.03  1.00    1.20  1.06    7.86e-04  3.43e-03
      2049     3    1.01  1.00    0.98  1.01    9.84e-04  4.65e-03
      8193     3    0.99  1.00    1.22  1.00    1.12e-03  5.14e-03
     16385     3    1.00  1.00    1.05  1.00    1.26e-03  5.86e-03
  bf16
       513     3    1.00  1.01    1.06  1.05    6.43e-03  3.83e-02
      2049     3    1.01  1.01    0.98  1.01    7.13e-03  3.87e-02
      8193     3    1.02  1.00    1.12  1.01    8.66e-03  4.41e-02
     16385     3    1.02  1.00    1.04  1.00    9.73e-03  4.25e-02
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import error_model as em
import per_token_reference as ptr
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu

K = 16                               # exact modes (fp32, fp16x3): x the float32 oracle's own per-token error
K16 = 4                              # 16-bit modes (fp16c, fp16, bf16): x the CPU error model's per-token error
B = 3                                # odd: one unit of the packed transform holds a single read

# (L, pads on read 1): see the module docstring for what each length reaches
SHAPES = [(L, 3) for L in (1, 2, 65, 129, 257, 513, 1025, 2049, 4097, 300, 1000, 3000, 4098, 6000, 8193, 8194, 16385, 20000)]
SHAPES += [(1000, 300), (20000, 9000)]
F16C_FORCED = (257, 513, 1000)       # fp16c once more below its length switch (clm_set_f16c_min_len(1))
PLAIN16 = (513, 2049, 8193, 16385)   # fp16 and bf16


def _cases():
    out = []
    for L, pads in SHAPES:
        modes = ["fp32", "fp16x3"]
        if L >= 2049:
            modes.append("fp16c")
        if pads == 3 and L in F16C_FORCED:
            modes.append("fp16c-forced")
        if pads == 3 and L in PLAIN16:
            modes += ["fp16", "bf16"]
        out += [pytest.param(L, pads, m, id=f"{L}-pads{pads}-{m}") for m in modes]
    return out


def _ids(L: int, pads: int) -> np.ndarray:
    """Read 0: [PAD] up to its [SEP] (its pair partner, read 1, must not leak into it); read 1: `pads` pads; read 2: 3 pads"""
    ids, _ = ho.synthetic_batch(17, B, L - 1, seed=1000 + L)
    ids[0, : L - 1] = 4
    ids[1, : min(pads, L - 1)] = 4
    ids[2, : min(3, L - 1)] = 4
    return ids


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0, head_scale=3.0)


@pytest.fixture(scope="module")
def engines(sd, built_lib):
    from chimeralm_amd.engine import Engine

    made: dict = {}

    def get(mode):
        if mode not in made:
            e = Engine("cuda:0", precision=mode.split("-")[0], chunk_reads=4)          # >= B: "h" keeps the whole batch
            e.load_state_dict(sd)
            if mode == "fp16c-forced":
                e.set_f16c_min_len(1)
            made[mode] = e
        return made[mode]

    yield get
    for e in made.values():
        e.close()


_ORACLE: dict = {}                   # (L, pads) -> (ids, truth, float32 yardstick); the cases of a shape follow each other


def _oracle(L, pads, sd):
    if (L, pads) not in _ORACLE:
        _ORACLE.clear()              # (3 x 20,000 x 256 float64 rows of four blocks: one shape at a time)
        ids = _ids(L, pads)
        ref = ptr.truth(ids, sd)
        _ORACLE[(L, pads)] = (ids, ref, ptr.yardstick(ids, sd, ref))
    return _ORACLE[(L, pads)]


def _model_yardstick(mode, ids, sd, ref, block):
    trace: dict = {}
    with torch.no_grad():
        em.forward(ids.astype(np.int64), sd, em.ENGINE_MODES[mode], trace=trace)
    return ptr.yardstick_of(ptr._trace_rows(trace), ref, block)


def _rows_16bit(ids: np.ndarray) -> np.ndarray | None:
    """The rows a 16-bit forward leaves unwritten in `h`: with [PAD]-prefix skipping (clm_api.hip plan_chunk: L >= 256) the tile
    list of read b starts one tile before its first non-prefix tile (pad_prefix.hip tile_list_kernel: start = p0 - 1, p0 =
    min(leading pads, Lmain) / 128, Lmain = L - 1 when the last token is peeled), and no kernel writes the tiles before it"""
    Bn, L = ids.shape
    if L < 256:
        return None
    Lmain = L - 1 if L % 128 == 1 else L
    keep = np.ones((Bn, L), bool)
    for b in range(Bn):
        lead = int(np.argmax(ids[b] != 4)) if (ids[b] != 4).any() else L
        p0 = min(lead, Lmain) // 128
        keep[b, : 128 * max(p0 - 1, 0)] = False
    return keep


@pytest.mark.parametrize("L,pads,mode", _cases())
def test_every_token_against_the_fp64_oracle(engines, sd, L, pads, mode):
    ids, ref, yard32 = _oracle(L, pads, sd)
    e = engines(mode)
    prec = mode.split("-")[0]
    ran = e.effective_precision(L)
    assert ran == prec, f"{mode} at {L} tokens runs {ran}"
    e.forward(torch.from_numpy(ids).cuda())                       # a full forward: no debug stop, no CLM_DEBUG
    got_h, got_s = e.debug_fetch("h", (B, L, 256)), e.debug_fetch("scores", (B, L))
    if prec in ("fp32", "fp16x3"):
        yard, k, rows = yard32, K, None                           # block 3's rows, every one of them (see the docstring)
    else:
        yard, k, rows = _model_yardstick(prec, ids, sd, ref, block=2), K16, _rows_16bit(ids)
        left = 0 if rows is None else int((~rows).sum())
        assert left % 128 == 0                                    # whole prefix tiles and nothing else
    r = ptr.ratios(got_h, got_s, ref, yard, rows)
    print(f"PER_TOKEN {mode:12s} L {L:5d} pads {pads:4d}: hidden max {r['h_max']:6.2f} rms {r['h_rms']:6.2f}   "
          f"scores max {r['s_max']:6.2f} rms {r['s_rms']:6.2f}   (yardstick: hidden {yard.hidden.max():.2e}, scores {yard.scores.max():.2e})")
    ptr.assert_per_token(got_h, got_s, ids, sd, k, rows, ref=ref, yard=yard, classes=prec not in ("fp32", "fp16x3"))
