"""The DNAConvNet forward (csrc/cnn.hip + tail32.hip's cnn_gemm7_kernel) stage by stage, in plain torch, for
tests/test_gpu_cnn_stages.py and tests/test_cnn_stage_host.py.  Written from tests/cnn_reference.py's formulas, which
tests/golden/cnn_golden.npz pins to the reference module.

One function per stage, each mapping that stage's INPUT to its output in the dtype of the input: evaluated in float64 on the engine's
own fetched input it is the reference of that stage alone (an error made upstream does not count against it); evaluated in float32 on
the CPU on the same input it is the yardstick, the error the same formulas have in the engine's number format.  `lin` replaces the
plain product of a block's convolution, taken over the 7 x 256 im2col rows (the fp16x3 split model, tests/error_model.py x3_linear);
`pad` replaces the zero rows a "same" convolution sees outside the read (the planted defects of tests/test_cnn_stage_host.py).

Stages and the buffers they connect (clm_cnn_debug_fetch names, include/chimeralm_hip.h):
    block0       ids                  -> "block0" [B, L/4, 256]     cnn_block0_kernel: embedding, then `block`
    block        rows [B, Lin, 256]   -> "block1" [B, L/16, 256]    cnn_gemm7_kernel<false, *>: Conv1d(k 7, "same") + eval BatchNorm +
                                                                    erf-GELU + MaxPool1d(4)
    block, tile_sums  "block1"        -> "partial" [B, tiles, 256]  cnn_gemm7_kernel<true, *>: block 2's pooled rows, never stored, summed
                                                                    in groups of 16
    pooled_from  "partial"            -> "pooled" [B, 256]          cnn_head_kernel: the partials added in order, over L/64
    head         "pooled"             -> logits [B, 2]              cnn_head_kernel: fc.0, BatchNorm, GELU, fc.4
`statistic`, `read_stats`, `check` and `FLOOR` are tests/tf_stage_reference.py's: the comparison is the same for every net.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import cnn_reference as cr
from tf_stage_reference import FLOOR, check, read_stats, statistic  # noqa: F401  (re-exported: the tests take them from here)

D, KW, HALO, POOL = 256, 7, 3, 4
BN_EPS = 1e-5
PT0 = 128                          # block 0: pooled positions per workgroup, two halves of 64 (cnn.hip)
TILE = 64                          # blocks 1 and 2: input rows per tile of cnn_gemm7_kernel (16 pooled rows)
ROWS2 = 16                         # block 2: pooled rows per partial


def weights(sd: dict, dtype) -> dict:
    return {k: v.detach().to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


# ------------------------------------------------------------------------------------------------------------- the stages
def zero_pad(x: torch.Tensor) -> torch.Tensor:
    """[B, Lin, 256] -> [B, Lin + 6, 256]: what a "same" convolution of width 7 sees, three zero rows on either side of every read."""
    return F.pad(x, (0, 0, HALO, HALO))


def im2col(xp: torch.Tensor) -> torch.Tensor:
    """Padded rows [B, Lin + 6, 256] -> [B, Lin, 7 x 256]: column dk x 256 + ci of row t is xp[t + dk][ci]."""
    Lin = xp.shape[1] - 2 * HALO
    return torch.cat([xp[:, dk:dk + Lin] for dk in range(KW)], dim=-1)


def conv_matrix(W: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [co, ci, dk] -> [co, 7 x 256] in im2col's column order."""
    return W.permute(0, 2, 1).reshape(W.shape[0], -1)


def block(w: dict, i: int, x_rows: torch.Tensor, lin=None, pad=zero_pad) -> torch.Tensor:
    """Block i on the token-major rows x [B, Lin, 256]: [B, Lin // 4, 256].  Trailing rows past 4 (Lin // 4) are dropped by the pool,
    but the last kept window still sees them as its right neighbours."""
    p = f"conv_blocks.{i}."
    xp = pad(x_rows)
    if lin is None:
        y = F.conv1d(xp.transpose(1, 2), w[p + "0.weight"], w[p + "0.bias"])
    else:
        y = (lin(im2col(xp), conv_matrix(w[p + "0.weight"])).to(x_rows.dtype) + w[p + "0.bias"]).transpose(1, 2)
    y = F.batch_norm(y, w[p + "1.running_mean"], w[p + "1.running_var"], w[p + "1.weight"], w[p + "1.bias"], training=False, eps=BN_EPS)
    return F.max_pool1d(F.gelu(y), POOL).transpose(1, 2).contiguous()


def block0(w: dict, ids: torch.Tensor, pad=zero_pad) -> torch.Tensor:
    """Block 0 on the embedding rows (a [PAD] row is an ordinary row; outside the read there is nothing)."""
    return block(w, 0, w["embedding.weight"][ids], pad=pad)


def tile_sums(rows2: torch.Tensor) -> torch.Tensor:
    """Block 2's pooled rows [B, L64, 256] summed in groups of 16: [B, ceil(L64 / 16), 256]; the last group sums the rows there are."""
    B, L64, C = rows2.shape
    tiles = -(-L64 // ROWS2)
    return F.pad(rows2, (0, 0, 0, tiles * ROWS2 - L64)).reshape(B, tiles, ROWS2, C).sum(dim=2)


def pooled_from(partial: torch.Tensor, L64: int) -> torch.Tensor:
    """[B, tiles, 256] -> [B, 256]: the partials added one after the other, first to last, then divided by L64 (cnn_head_kernel's
    order; in float32 it is that kernel's arithmetic)."""
    s = torch.zeros_like(partial[:, 0])
    for t in range(partial.shape[1]):
        s = s + partial[:, t]
    return s / float(L64)


def head(w: dict, pooled: torch.Tensor) -> torch.Tensor:
    h = F.linear(pooled, w["fc.0.weight"], w["fc.0.bias"])
    h = F.gelu(F.batch_norm(h, w["fc.1.running_mean"], w["fc.1.running_var"], w["fc.1.weight"], w["fc.1.bias"], training=False, eps=BN_EPS))
    return F.linear(h, w["fc.4.weight"], w["fc.4.bias"])


def forward(sd: dict, ids, dtype=torch.float64, trace: dict | None = None, replace: dict | None = None) -> torch.Tensor:
    """Logits of the net chained from the stages (tests/test_cnn_stage_host.py holds it to tests/cnn_reference.py); `trace` receives
    "block0", "block1", "block2" (the rows block 2 never stores), "partial", "pooled".  `replace`: name -> f(w, input) computing that
    buffer instead of the stage (the planted defects of tests/test_cnn_stage_host.py); everything behind it runs on what f returned."""
    w = weights(sd, dtype)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    tr = {} if trace is None else trace
    rp = replace or {}
    tr["block0"] = rp["block0"](w, ids) if "block0" in rp else block0(w, ids)
    tr["block1"] = rp["block1"](w, tr["block0"]) if "block1" in rp else block(w, 1, tr["block0"])
    tr["block2"] = rp["block2"](w, tr["block1"]) if "block2" in rp else block(w, 2, tr["block1"])
    tr["partial"] = rp["partial"](w, tr["block1"]) if "partial" in rp else tile_sums(tr["block2"])
    tr["pooled"] = pooled_from(tr["partial"], tr["block2"].shape[1])
    return head(w, tr["pooled"])


# ------------------------------------------------------------------------------------------------------------- geometry
def geometry(L: int) -> dict:
    """What a read of L tokens reaches in the three kernels.  Block 0: `wg0` workgroups of 128 pooled positions, thread halves of 64;
    `last_wg0` positions in the last workgroup, `last_half0` of them in its second half.  Blocks 1 and 2 (Lin = L4, L16): `tiles`
    tiles of 64 input rows over the 4 Lout rows that feed a window; `trail` real rows behind the last window (L % 4 in block 0);
    `halo` of them lie in the last tile's right halo, rows t0 + 64 .. t0 + 66 (the others inside the tile).  `last_rows2`: pooled
    rows the last partial sums."""
    L4, L16, L64 = L // 4, L // 16, L // 64
    g = {"L4": L4, "L16": L16, "L64": L64, "tiles2": -(-L64 // ROWS2), "trail0": L - 4 * L4}
    g["wg0"] = -(-L4 // PT0)
    g["last_wg0"] = L4 - PT0 * (g["wg0"] - 1)
    g["last_half0"] = max(0, g["last_wg0"] - PT0 // 2)
    for lvl, (Lin, Lout) in ((1, (L4, L16)), (2, (L16, L64))):
        tiles = -(-4 * Lout // TILE)
        g[f"tiles{lvl}_x"] = tiles
        g[f"last_out{lvl}"] = Lout - (TILE // POOL) * (tiles - 1)
        g[f"trail{lvl}"] = Lin - 4 * Lout
        g[f"halo{lvl}"] = min(HALO, max(0, Lin - TILE * tiles))
    assert g["tiles2_x"] == g["tiles2"]
    g["last_rows2"] = g["last_out2"]
    return g


# ------------------------------------------------------------------------------------------------------------- nets, reads, cases
def stage_ids(seed: int, B: int, L: int) -> np.ndarray:
    """Bases from cnn_reference.synthetic_ids.  Read 0 left-padded with [PAD] = 4 up to its last token: constant windows, exact ties in
    every max-pool; read 1 without pads; read 2 with 3 pads and one N."""
    ids = cr.synthetic_ids(seed, B, L)
    ids[ids == 11] = 7                                         # (the one N is placed, not drawn; no drawn pads either)
    ids[ids == 4] = 8
    ids[0, :L - 1] = 4
    if B > 2:
        ids[2, :3] = 4
        ids[2, L // 2] = 11
    return ids


SEED_SHAPES, SEED_REGIMES = 64, 6                              # cnn_reference.make_cnn_state_dict seeds of the shape and regime cases
# (B, L) of the GPU cases: the smallest lengths at which each path differs; what each reaches is GEOMETRY's claim, which
# tests/test_cnn_stage_host.py computes from L
SHAPES = [(3, 64), (1, 64), (3, 67), (3, 127), (3, 259), (3, 263), (3, 271), (3, 272), (3, 515), (3, 519), (3, 1039), (3, 1075),
          (3, 1091), (3, 2099)]
GEOMETRY = {
    64: dict(L4=16, L16=4, L64=1, wg0=1, tiles1_x=1, tiles2=1, trail0=0, trail1=0, trail2=0, last_rows2=1),    # one tile, one pooled row
    67: dict(L4=16, L16=4, L64=1, trail0=3, trail1=0, trail2=0),                                               # tokens 64 - 66 real neighbours
    127: dict(L4=31, L16=7, L64=1, trail0=3, trail1=3, trail2=3, halo1=0, halo2=0, tiles1_x=1, tiles2=1),      # every level ragged
    259: dict(L4=64, L16=16, L64=4, tiles1_x=1, last_out1=16, trail1=0, halo1=0, wg0=1, last_half0=0),         # block 1 one whole tile, zero halo
    263: dict(L4=65, L16=16, L64=4, tiles1_x=1, trail1=1, halo1=1, last_half0=1),                              # one real halo row
    271: dict(L4=67, L16=16, L64=4, tiles1_x=1, trail1=3, halo1=3),                                            # three, no second tile
    272: dict(L4=68, L16=17, L64=4, tiles1_x=2, last_out1=1, trail1=0),                                        # second tile: one pooled row
    515: dict(L4=128, L16=32, L64=8, wg0=1, last_wg0=128, last_half0=64),                                      # block 0 exactly one workgroup
    519: dict(L4=129, L16=32, L64=8, wg0=2, last_wg0=1, last_half0=0, tiles1_x=2, trail1=1, halo1=1),          # its second holds one position
    1039: dict(L4=259, L16=64, L64=16, tiles2=1, last_rows2=16, trail2=0, halo2=0),                            # block 2 one whole tile
    1075: dict(L4=268, L16=67, L64=16, tiles2=1, last_rows2=16, trail2=3, halo2=3),                            # three real halo rows
    1091: dict(L4=272, L16=68, L64=17, tiles2=2, last_rows2=1, trail2=0),                                      # second partial sums one row
    2099: dict(L4=524, L16=131, L64=32, wg0=5, last_wg0=12, tiles1_x=9, last_out1=3, trail0=3, trail1=0, trail2=3, halo2=3, tiles2=2),
}
REGIME_SHAPE = (3, 1075)
REGIMES = ("allneg", "deep", "act2^-4", "act2^-8", "act2^-12")
SCALE_REGIMES = REGIMES[2:]


def regime_state_dict(name: str, seed: int = SEED_REGIMES) -> dict:
    """A seeded net pushed into a regime through its weights:
    unit      as seeded (act2^0 of the scale axis);
    allneg    every block's BatchNorm weight negative: the max-pool picks the smallest normalised value;
    deep      every block's BatchNorm bias -1.5: the pre-activations sit in GELU's non-monotonic range, row maxima of about 0.16;
    act2^-k   block 0's BatchNorm weight and bias x 2^-k: block 1's input is small, the fp16x3 lo halves are fp16 subnormals."""
    sd = cr.make_cnn_state_dict(seed)
    if name == "unit":
        pass
    elif name == "allneg":
        for i in range(3):
            sd[f"conv_blocks.{i}.1.weight"] = -sd[f"conv_blocks.{i}.1.weight"].abs()
    elif name == "deep":
        for i in range(3):
            sd[f"conv_blocks.{i}.1.bias"] = torch.full_like(sd[f"conv_blocks.{i}.1.bias"], -1.5)
    elif name.startswith("act2^-"):
        s = 2.0 ** -int(name[6:])
        for k in ("weight", "bias"):
            sd[f"conv_blocks.0.1.{k}"] = sd[f"conv_blocks.0.1.{k}"] * s
    else:
        raise ValueError(name)
    return sd
