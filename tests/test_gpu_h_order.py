"""GPU (MI355X): the residual stream handed from tail launch to tail launch in register order (gemm16.hip HREG, ChunkPlan::hreg).

Where every 128-token tile of a fused 16-bit forward is whole, the tail kernels keep h inside each tile's 128 KiB in the order of
the accumulator registers instead of rows.  That is a permutation of storage and nothing else, so against the same engine held to
row order (CLM_DEBUG=row_h) the logits are the same bits, and clm_debug_fetch("h") -- which un-permutes -- returns the same rows.
CLM_DEBUG is read when a handle is created: each setting runs in a child process of its own (tests/h_order_child.py), once per
module."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from h_order_child import CASES
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("h_order")
    out = {}
    for name, debug in (("default", None), ("row_h", "row_h")):
        env = {k: v for k, v in os.environ.items() if k != "CLM_DEBUG"}
        if debug:
            env["CLM_DEBUG"] = debug
        r = subprocess.run([sys.executable, str(REPO / "tests" / "h_order_child.py"), str(d / f"{name}.npz")], capture_output=True,
                           text=True, env=env, cwd=str(REPO), timeout=240)
        assert r.returncode == 0, f"{name}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        out[name] = dict(np.load(d / f"{name}.npz"))
    return out


@pytest.mark.parametrize("prec,B,L", CASES)
def test_logits_are_the_same_bits_in_either_order(runs, prec, B, L):
    """257 / 256 / 385 tokens run in register order (whole tiles, with and without the peeled token, odd batch, three tiles);
    300 tokens have a partial last tile and fall back to rows in both processes."""
    k = f"logits_{prec}_{B}x{L}"
    assert np.isfinite(runs["default"][k]).all()
    assert np.array_equal(runs["default"][k], runs["row_h"][k])


@pytest.mark.parametrize("prec,B,L", CASES)
def test_logits_stay_within_the_parity_tolerance_of_the_exact_engine(runs, prec, B, L):
    got, ref = runs["default"][f"logits_{prec}_{B}x{L}"], runs["default"][f"exact_{prec}_{B}x{L}"]
    err = float(np.abs(got - ref).max())
    print(f"{prec} {B} x {L}: |logits - exact fp32 engine| {err:.2e} (tolerance {TOL[prec]})")
    assert err <= TOL[prec], err


def test_a_batch_with_a_skipped_pad_tile_is_the_same_bits(runs):
    """513 tokens, one read with a 300-token [PAD] prefix: its first tile is in no launch's list, in either order."""
    assert np.isfinite(runs["default"]["logits_pad"]).all()
    assert np.array_equal(runs["default"]["logits_pad"], runs["row_h"]["logits_pad"])


@pytest.mark.parametrize("prec", ["fp16c", "fp16"])
def test_debug_fetch_returns_rows_in_either_order(runs, prec):
    """After a complete fused forward at 257 tokens h holds what the last storing block left: the fetch un-permutes the two whole
    tiles (rows t < Lmain = 256) of the register-order run."""
    a, b = runs["default"][f"h_{prec}_3x257"], runs["row_h"][f"h_{prec}_3x257"]
    assert a.shape == (3, 257, 256) and np.isfinite(a[:, :256]).all()
    assert np.array_equal(a[:, :256], b[:, :256])
    assert np.abs(a[:, :256]).max() > 0
