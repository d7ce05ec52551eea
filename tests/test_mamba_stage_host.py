"""The stage references of tests/test_gpu_mamba_stages.py without a GPU: composed, the stages are the fp64 forward the other Mamba
tests trust; the chunked scan equals the recurrence in the decay regimes the GPU tests add; the float32 chunked yardstick stays
usable there; the fp16x3 split model (tests/error_model.py) reproduces the activation-scale figures the stage tests were written
around."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import error_model as em
import mamba_reference as mr
import mamba_stage_reference as S
from mamba_stage_reference import REGIMES, regime_state_dict

# embedding.weight x 2^-k -> max |logit error| of the split format against fp64 (mambasp, 2 layers, seed 26, the reads of
# test_gpu_mamba.py::test_fp16x3_range_guard_and_nonfinite_rerun), as first measured with a numpy float16 emulation
SPLIT_TABLE = {0: 6.2e-7, 4: 6.1e-6, 8: 6.3e-5, 16: 2.3e-4, 20: 1.1e-4}


@pytest.mark.parametrize("L", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("variant,masked", [("mamba", False), ("mamba", True), ("mambasp", False)])
def test_composed_stages_equal_the_fp64_forward(variant, masked, L):
    sd = mr.make_mamba_state_dict(variant, 40, n_layers=2, d_model=256, expand=1, d_state=16, model_max_length=256)
    ids = mr.synthetic_ids(4000 + L, 2, L, pads=min(5, L - 1))
    mask = None
    if masked:
        mask = (np.random.default_rng(L).random((2, L)) > 0.2).astype(np.float32)
        mask[1, L // 2:] = 0.0
    tr, st = {}, {}
    want = mr.mamba_forward_fp64(variant, sd, ids, mask=mask, trace=tr)
    got = S.forward(variant, sd, ids, mask=mask, trace=st)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # ... and one layer of them equals mamba2_fp64 on the same input
    w = {k: v.double() for k, v in sd.items()}
    m = None if mask is None else torch.from_numpy(mask).double()
    h = S.front(variant, w, torch.from_numpy(ids), m)
    assert float((h - tr["front"]).abs().max()) <= 1e-12
    p = S.layer_params(variant, sd, 0, torch.float64)
    out = S.layer(p, h)
    assert float((out - h - mr.mamba2_fp64(p, h)).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    if m is not None:
        out = out * m[..., None]
    assert float((out - tr["layer0"]).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    pooled = S.pooled_of(st["part"], L)
    assert float((pooled - tr["pooled"]).abs().max()) <= 1e-12 * max(1.0, float(pooled.abs().max()))


def test_fully_masked_tile_pools_to_zero():
    h = torch.randn(1, 130, 8, dtype=torch.float64)
    h[:, 128:] = 0.0
    part = S.partials(h)
    assert part.shape == (1, 3, 2, 8) and float(part[:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("regime", REGIMES)
def test_regimes_chunked_equals_sequential_and_the_fp32_yardstick_holds(regime):
    sd = regime_state_dict(regime)
    ids = mr.synthetic_ids(3100, 2, 200, pads=0)
    p64 = S.layer_params("mambasp", sd, 0, torch.float64)
    D = S.dims_of(p64)
    h = torch.nn.functional.embedding(torch.from_numpy(ids), sd["embedding.weight"])
    zx32 = S.in_proj(S.layer_params("mambasp", sd, 0, torch.float32), h)           # (a float32 input, as the engine's is)
    zx = zx32.double()
    xc = S.conv(p64, zx)
    dt = zx[..., D.dt0:]
    print(f"{regime}: dt in [{float(dt.min()):.2e}, {float(dt.max()):.2e}], A = {float(torch.exp(p64['A_log']).max()):g}, "
          f"largest token-to-token dt ratio {float((dt[:, 1:] / dt[:, :-1]).max()):.1e}, "
          f"chunk decay exp(s_63) down to {float(torch.exp((dt[:, :64] * -torch.exp(p64['A_log'])).sum(1)).min()):.1e}")
    x, Bm, Cm = xc.split([D.di, D.N, D.N], dim=-1)
    A = -torch.exp(p64["A_log"])
    xs = x.reshape(2, 200, D.H, 64)
    seq, ch = mr.scan_sequential(xs, dt, A, Bm, Cm, p64["D"]), mr.scan_chunked(xs, dt, A, Bm, Cm, p64["D"])
    assert torch.isfinite(ch).all()
    assert float((ch - seq).abs().max()) <= 1e-10 * max(1.0, float(seq.abs().max()))
    # the float32 chunked yardstick on the same input: finite, and a usable yardstick (below 1e-3)
    g64, q64 = S.scan(p64, zx, xc)
    g32, q32 = S.scan(S.layer_params("mambasp", sd, 0, torch.float32), zx32, xc.float())
    assert torch.isfinite(g32).all() and torch.isfinite(q32).all()
    sg, sq = S.statistic(g32, g64, "row", groups=D.H), S.statistic(q32, q64, "row", groups=D.H)
    print(f"{regime}: float32 chunked yardstick g max {float(sg.max()):.2e} rms {float(sg.pow(2).mean().sqrt()):.2e}, "
          f"ssq max {float(sq.max()):.2e}")
    assert float(sg.max()) < 1e-3 and float(sq.max()) < 1e-3
    if regime == "steep":
        s63 = (dt[:, :64] * A).sum(1)
        assert float(torch.exp(s63.float()).min()) == 0.0          # exp(s_63) underflows in float32 ...
        assert float(g64.abs().amax(-1).min()) > 0.0               # ... and every token keeps its diagonal term
    if regime == "mixed":
        assert float((dt[:, 1:] / dt[:, :-1]).max()) >= 1e3


def test_split_model_reproduces_the_scale_table():
    ids = mr.synthetic_ids(2500, 2, 300)
    sd0 = mr.make_mamba_state_dict("mambasp", 26, n_layers=2)
    for k, want in SPLIT_TABLE.items():
        sd = {**sd0, "embedding.weight": sd0["embedding.weight"] * 2.0 ** -k}
        ref = em.mamba_x3_forward("mambasp", sd, ids, exact=True)
        assert float((ref - mr.mamba_forward_fp64("mambasp", sd, ids)).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
        err = float((em.mamba_x3_forward("mambasp", sd, ids) - ref).abs().max())
        print(f"embedding x 2^-{k}: split model {err:.2e}, table {want:.2e}")
        assert want / 2 <= err <= want * 2, (k, err)
        # exact fp32 does not care: its products carry the scale in the exponent
        e32 = float((S.forward("mambasp", sd, ids, dtype=torch.float32).double() - ref).abs().max())
        assert e32 < 1e-4 * max(1.0, float(ref.abs().max())), (k, e32)


def test_split_is_the_documented_one():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -10 * (1 + 2.0 ** -11 + 2.0 ** -12), 70000.0, 2.0 ** -26], dtype=torch.float64)
    hi, lo = em.x3_split(v)
    assert hi.tolist()[0] == 1.0 and lo.tolist()[0] == 0.0
    assert float(hi[1] + lo[1]) == 1.0 + 2.0 ** -11 + 2.0 ** -20                  # 21 bits survive at unit scale
    assert float(lo[2]) == 2.0 ** -21 + 2.0 ** -22 or abs(float(hi[2] + lo[2] - v[2])) <= 2.0 ** -25   # subnormal lo: absolute 2^-25
    assert float(hi[3]) == 65504.0 and float(lo[3]) == 70000.0 - 65504.0          # saturating, not inf
    assert float(hi[4]) == 0.0 and float(lo[4]) == 0.0                            # below half of fp16's smallest subnormal
    fh, fl = em.x3_split(v, flush=True)
    assert float(fl[2]) == 0.0 and float(fh[2]) == float(hi[2])
