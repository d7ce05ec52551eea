"""GPU (MI355X): the head fine-tune -- the pooling kernels (csrc/pool_train.hip) on given rows against the fp64 formulas, their
determinism, the rows the engine hands out, the module's gradients, a short fit and the errors.

The bound of every comparison: err = max |engine - fp64| / max |fp64| must be <= max(8 x the same error of the formulas evaluated in
float32 on the CPU for the same inputs, 32 x 2^-24).  The factor 8 covers the kernel's three nested levels of partial sums (tile,
workgroup, grid) against torch's one; the floor of 32 fp32 roundoffs keeps a lucky CPU run from failing the test.

The reference takes the normal cdf as 0.5 erfc(-u / sqrt 2) in both precisions (tests/headtrain_reference.py `cdf`), as the kernel does.
db2 keeps dw2's bound and scale: the row file's sum |ds_t| denominator gives a LOOSER bound at nine of this file's ten shapes (float32
yardstick on the CPU: 2.4e-5 - 1.3e-4 against 3.9e-6 - 1.8e-5; tighter only at 2 x 200 with w2 x 40).  tests/test_gpu_headtrain_rows.py
holds the same kernels row by row.

CLM_HEADTRAIN_PARITY=<file> appends the measured ratios of the parity cases to that file (profiles/headtrain_parity.txt is one).
"""
from __future__ import annotations

import copy
import os
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import headtrain_reference as hr
from oracle import hyena_oracle as ho

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PARQUET = REPO / "tests" / "golden" / "tests.parquet"
FLOOR = 32 * 2.0 ** -24
NAMES = ("dW1", "db1", "dw2")
POOL_KEYS = ("attention.0.weight", "attention.0.bias", "attention.2.weight", "attention.2.bias")


@pytest.fixture(scope="module")
def sd():
    return ho.make_state_dict(0)


@pytest.fixture(scope="module")
def engines(sd, built_lib):
    from chimeralm_amd.engine import Engine

    out = {}
    for prec in ("fp32", "fp16x3"):
        out[prec] = Engine("cuda:0", precision=prec, chunk_reads=4)
        out[prec].load_state_dict(sd)
    yield out
    for e in out.values():
        e.close()


def _bound(err32: float) -> float:
    return max(8.0 * err32, FLOOR)


_cases: dict = {}


def _case(B, L, scale, sd):
    """Inputs, the fp64 reference and the float32-on-CPU yardstick of one shape: computed once, shared, never changed."""
    key = (B, L, scale)
    if key not in _cases:
        c = hr.seeded_case(B, L, seed=1, w2_scale=scale, sd=sd)
        args = (c["rows"], c["lnf_g"], c["lnf_b"], c["w1"], c["b1"], c["w2"], c["b2"], c["dpooled"])
        f64, g64 = hr.pool_grads(*args, torch.float64)
        f32, g32 = hr.pool_grads(*args, torch.float32)
        c["ref"] = {"pooled": f64["pooled"], "scores": f64["scores"], "dW1": g64[0], "db1": g64[1], "dw2": g64[2], "db2": g64[3]}
        c["err32"] = {"pooled": hr.rel_err(f32["pooled"], f64["pooled"]), **{n: hr.rel_err(g32[i], g64[i]) for i, n in enumerate(NAMES)}}
        _cases[key] = c
    return _cases[key]


def _run(eng, c, out=None, beta=0.0, rows=None, dpooled=None):
    dev = eng.device
    rows = (c["rows"] if rows is None else rows).to(dev)
    w1, b1, w2, b2 = (c[k].to(dev).contiguous() for k in ("w1", "b1", "w2", "b2"))
    scores, stats, pooled = eng.pool_forward(rows, w1, b1, w2.view(-1), b2)
    grads = eng.pool_backward(rows, w1, b1, w2.view(-1), scores, stats, pooled, (c["dpooled"] if dpooled is None else dpooled).to(dev),
                              out=out, beta=beta)
    return pooled, grads


SHAPES = [(B, L, 1.0) for L in (1, 63, 64, 65, 200) for B in (1, 3)] + [(5, 4097, 1.0), (2, 200, 40.0)]


@pytest.mark.parametrize("B,L,scale", SHAPES)
def test_kernel_parity_on_given_rows(engines, sd, B, L, scale):
    """Odd sizes either side of the 64-token tile, one and several reads, 325 tiles on the 256-workgroup grid (workgroups own
    several tiles), and softmax weight 1.000 on one position (w2 x 40)."""
    c = _case(B, L, scale, sd)
    pooled, grads = _run(engines["fp32"], c)
    got = {"pooled": pooled.cpu(), "dW1": grads[0].cpu(), "db1": grads[1].cpu(), "dw2": grads[2].cpu(), "db2": grads[3].cpu()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    lines, fails = [], []
    for n in ("pooled",) + NAMES:
        if L == 1 and n != "pooled":
            continue
        err, bound = hr.rel_err(got[n], c["ref"][n]), _bound(c["err32"][n])
        lines.append(f"B={B} L={L} w2x{scale:g} {n}: err {err:.3e}  cpu-f32 err {c['err32'][n]:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}")
        if not err <= bound:
            fails.append(lines[-1])
    db2, db2_bound = abs(float(got["db2"])), _bound(c["err32"]["dw2"]) * float(c["ref"]["dw2"].abs().max())
    lines.append(f"B={B} L={L} w2x{scale:g} |db2| {db2:.3e}  bound {db2_bound:.3e}")
    if L == 1:          # one position: softmax weight 1, every gradient of the pooling is 0
        for n in NAMES + ("db2",):
            worst = float(got[n].abs().max())
            lines.append(f"B={B} L=1 max |{n}| {worst:.3e}  floor {FLOOR:.3e}")
            if not worst <= FLOOR:
                fails.append(lines[-1])
    elif not db2 <= db2_bound:
        fails.append(lines[-1])
    print("\n".join(lines))
    if os.environ.get("CLM_HEADTRAIN_PARITY"):
        with open(os.environ["CLM_HEADTRAIN_PARITY"], "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,L", [(3, 200), (5, 4097)])
def test_backward_is_deterministic_and_accumulates(engines, sd, B, L):
    eng = engines["fp32"]
    c = _case(B, L, 1.0, sd)
    p1, g1 = _run(eng, c)
    p2, g2 = _run(eng, c)
    assert torch.equal(p1, p2) and all(torch.equal(a, b) for a, b in zip(g1, g2))           # two calls: equal bits
    zeros = tuple(torch.zeros_like(g) for g in g1)
    _, g3 = _run(eng, c, out=zeros, beta=1.0)
    assert all(torch.equal(a, b) for a, b in zip(g1, g3))                                     # beta = 1 on zeros = beta = 0
    # two micro-batches accumulated against the whole batch: the bound of the parity test
    k = B // 2
    out = tuple(torch.full_like(g, float("nan")) for g in g1)                                 # (beta = 0 does not read them)
    _run(eng, c, out=out, beta=0.0, rows=c["rows"][:k], dpooled=c["dpooled"][:k])
    _run(eng, c, out=out, beta=1.0, rows=c["rows"][k:], dpooled=c["dpooled"][k:])
    for i, n in enumerate(NAMES):
        err = hr.rel_err(out[i], c["ref"][n])
        print(f"B={B} L={L} accumulated {n}: err {err:.3e} bound {_bound(c['err32'][n]):.3e}")
        assert err <= _bound(c["err32"][n]), n


def _ids(B, L, pad_first=0):
    ids, _ = ho.synthetic_batch(3, B, L - 1, seed=11)
    ids = torch.from_numpy(ids).long()
    if pad_first:
        ids[0, :pad_first] = 4
    return ids


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("B,L,pad", [(3, 200, 66), (2, 65, 0), (2, 400, 260)])   # (the last: row 0's first two 128-token tiles come from the [PAD] table)
def test_rows_are_the_forwards_rows(engines, sd, prec, B, L, pad):
    eng = engines[prec]
    eng.forward(_ids(B, L, pad).cuda())
    gen = eng.rows_generation()
    rows = eng.rows()
    assert tuple(rows.shape) == (B, L, 256) and rows.dtype == torch.float32 and rows.is_cuda
    h = torch.from_numpy(eng.debug_fetch("h", (B, L, 256)))
    assert torch.equal(rows.cpu(), h)
    w = [sd[ho.HD + k].float().cuda().contiguous() for k in POOL_KEYS]
    scores, stats, pooled = eng.pool_forward(rows, w[0], w[1], w[2].view(-1), w[3])
    assert eng.rows_generation() == gen                      # the pooling calls leave the rows alone
    for name, got, shape in (("scores", scores, (B, L)), ("pooled", pooled, (B, 256))):
        want = torch.from_numpy(eng.debug_fetch(name, shape))
        err = hr.rel_err(got, want)
        print(f"{prec} {B}x{L} {name}: {err:.3e} (floor {FLOOR:.3e})")
        assert err <= FLOOR, name
    eng.forward(_ids(B, L, pad).cuda())
    assert eng.rows_generation() != gen


def _module(sd, freeze=True, dropout=0.0, chunk_reads=2):
    from chimeralm_amd.basic_module import ClassificationLit
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    lit = ClassificationLit(net=HyenaDna(2, BinarySequenceClassifier(256, dropout=dropout), freeze_backbone=freeze, precision="fp32",
                                         chunk_reads=chunk_reads, selfcheck=False),
                            optimizer=lambda params: torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01),
                            scheduler=lambda optimizer: torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.1, patience=10))
    lit.load_state_dict(sd, strict=True)
    return lit.cuda()


def _head_reference(net, rows, labels, dt):
    """Gradients of every head parameter: the formulas for the pooling, autograd for the MLP, on `rows`, in dtype dt on the CPU."""
    head = copy.deepcopy(net.head).cpu().to(dt)
    lnf = net.backbone.backbone.ln_f
    att0, att2 = head.attention[0], head.attention[2]
    fwd = hr.pool_forward(rows, lnf.weight.detach().cpu(), lnf.bias.detach().cpu(), att0.weight.detach(), att0.bias.detach(),
                          att2.weight.detach(), att2.bias.detach(), dt)
    pooled = fwd["pooled"].clone().requires_grad_(True)
    from chimeralm_amd.headtrain import head_mlp

    for p in head.parameters():
        p.grad = None
    F.cross_entropy(head_mlp(SimpleNamespace(head=head), pooled), labels).backward()
    dw1, db1, dw2, db2 = hr.pool_backward(fwd, att2.weight.detach(), pooled.grad)
    grads = {k: p.grad for k, p in head.named_parameters() if p.grad is not None}
    grads.update({"attention.0.weight": dw1, "attention.0.bias": db1, "attention.2.weight": dw2.reshape(1, -1), "attention.2.bias": db2.reshape(1)})
    return grads


def test_module_gradients(sd):
    lit = _module(sd)
    net = lit.net.train()
    ids, labels = _ids(5, 130, 40).cuda(), torch.tensor([0, 1, 1, 0, 1])
    logits = net(ids)                                        # three micro-batches: 2 + 2 + 1 reads
    assert logits.requires_grad and tuple(logits.shape) == (5, 2)
    F.cross_entropy(logits, labels.cuda()).backward()
    assert all(p.grad is None for p in net.backbone.parameters())
    # dropout 0: the training path (pooling kernels + torch MLP) computes what the inference kernels compute, to fp32 roundoff.  The
    # two sum the five dense layers (up to 512 terms each) in different orders: ~sqrt(512) = 23 roundoffs per layer, five layers and
    # the pooling -> 128 x 2^-24 of the largest logit (a wrong layer order would be off by the logits' own size)
    with torch.no_grad():
        infer = net.eval()(ids)
    net.train()
    gap = hr.rel_err(logits.detach(), infer)
    print(f"training-path logits against the inference kernels': {gap:.3e} (bound {128 * 2.0 ** -24:.3e})")
    assert gap <= 128 * 2.0 ** -24
    eng = net.engine(ids.device)
    rows = []
    for b0 in range(0, 5, 2):                                # the engine's own rows: backbone error stays out of the comparison
        eng.forward(ids[b0:b0 + 2])
        rows.append(eng.rows().cpu())
    rows = torch.cat(rows)
    g64, g32 = _head_reference(net, rows, labels, torch.float64), _head_reference(net, rows, labels, torch.float32)
    got = {k: p.grad.cpu() for k, p in net.head.named_parameters()}
    assert sorted(got) == sorted(g64)
    for k in sorted(got):
        if k == "attention.2.bias":                          # 0 in exact arithmetic
            bound = _bound(hr.rel_err(g32["attention.2.weight"], g64["attention.2.weight"])) * float(g64["attention.2.weight"].abs().max())
            assert abs(float(got[k])) <= bound, k
            continue
        err, bound = hr.rel_err(got[k], g64[k]), _bound(hr.rel_err(g32[k], g64[k]))
        print(f"{k}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, k
    # a backward issued after another forward raises and reads nothing
    for p in net.parameters():
        p.grad = None
    loss = F.cross_entropy(net(ids[:2]), labels[:2].cuda())
    with torch.no_grad():
        net(ids[:2])
    with pytest.raises(RuntimeError, match="another forward"):
        loss.backward()
    assert net.head.attention[0].weight.grad is None and net.head.attention[2].weight.grad is None
    # eval() afterwards: the inference path, bitwise what a module that never trained gives
    with torch.no_grad():
        after = net.eval()(ids).cpu()
        never = _module(sd, freeze=False).net.eval()(ids).cpu()
    assert not after.requires_grad and torch.equal(after, never)


def _fit(sd, out_dir):
    from chimeralm_amd import headtrain

    torch.manual_seed(0)
    lit = _module(sd, chunk_reads=4)
    hist = headtrain.fit_head(lit, (str(PARQUET), 0, 25), (str(PARQUET), 0, 25), out_dir, epochs=3, batch_size=8, lr=1e-3, seed=12345,
                              device="cuda:0")
    return lit, [{k: v for k, v in r.items() if k != "seconds"} for r in hist]


def test_fit_head_and_the_command(sd, tmp_path):
    from safetensors.torch import load_file
    from typer.testing import CliRunner

    from chimeralm_amd import lm
    from chimeralm_amd.__main__ import app

    lit, hist = _fit(sd, tmp_path / "a")
    print([(r["train/loss"], r["val/loss"], r["val/f1"]) for r in hist])
    assert hist[2]["train/loss"] < hist[0]["train/loss"]
    _, again = _fit(sd, tmp_path / "b")
    assert hist == again                                     # bitwise repeatable: every figure of every epoch ...
    a, b = load_file(str(tmp_path / "a" / "model.safetensors")), load_file(str(tmp_path / "b" / "model.safetensors"))
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)               # ... and the saved weights
    assert not torch.equal(a["net.head.classifier.0.weight"], sd["net.head.classifier.0.weight"])
    assert torch.equal(a["net.backbone.backbone.ln_f.weight"], sd["net.backbone.backbone.ln_f.weight"])
    ids = _ids(3, 300, 20).cuda()
    fresh = lm.ChimeraLM.from_pretrained(str(tmp_path / "a"), precision="fp32", selfcheck=False, chunk_reads=4).cuda()
    with torch.no_grad():
        assert torch.equal(fresh.net.eval()(ids), lit.net.eval()(ids))
    res = CliRunner().invoke(app, ["finetune", str(PARQUET), "-o", str(tmp_path / "cli"), "--epochs", "1", "-b", "8", "--precision", "fp32",
                                   "--weights", str(tmp_path / "a")], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert (tmp_path / "cli" / "model.safetensors").stat().st_size > 0
    assert len((tmp_path / "cli" / "metrics.tsv").read_text().splitlines()) == 2


def test_errors(sd, engines, built_lib):
    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import Engine, EngineError

    def code(fn):
        with pytest.raises(EngineError) as e:
            fn()
        return e.value.code

    small = Engine("cuda:0", precision="fp32", chunk_reads=2)
    try:
        small.load_state_dict(sd)
        assert code(small.rows) == N.E_STATE                 # no forward yet
        small.forward(_ids(3, 65).cuda())                    # two chunks: only the last one's rows are left
        assert code(small.rows) == N.E_STATE
        small.forward(_ids(2, 65).cuda())
        assert tuple(small.rows().shape) == (2, 65, 256)
    finally:
        small.close()
    f16c = Engine("cuda:0", precision="fp16c", chunk_reads=4)
    try:
        f16c.load_state_dict(sd)
        f16c.set_f16c_min_len(1)                             # (so that this short read runs the 16-bit kernels)
        f16c.forward(_ids(2, 200).cuda())
        assert code(f16c.rows) == N.E_UNSUPPORTED
    finally:
        f16c.close()
    eng = engines["fp32"]
    c = _case(1, 63, 1.0, sd)
    rows = c["rows"].cuda()
    w1, b1, w2, b2 = (c[k].cuda().contiguous() for k in ("w1", "b1", "w2", "b2"))
    assert code(lambda: eng.pool_forward(None, w1, b1, w2.view(-1), b2)) == N.E_INVALID
    assert code(lambda: eng.pool_forward(rows, None, b1, w2.view(-1), b2)) == N.E_INVALID
    assert code(lambda: eng.pool_forward(rows[:0], w1, b1, w2.view(-1), b2)) == N.E_INVALID
    assert code(lambda: eng.pool_forward(rows[:, :0], w1, b1, w2.view(-1), b2)) == N.E_INVALID
    scores, stats, pooled = eng.pool_forward(rows, w1, b1, w2.view(-1), b2)
    dp = c["dpooled"].cuda()
    assert code(lambda: eng.pool_backward(rows, w1, b1, w2.view(-1), scores, stats, pooled, None)) == N.E_INVALID
    assert code(lambda: eng.pool_backward(rows[:0], w1, b1, w2.view(-1), scores[:0], stats[:0], pooled[:0], dp[:0])) == N.E_INVALID
    out = tuple(torch.zeros(s, device="cuda") for s in ((256, 256), (256,), (256,), (1,)))
    assert code(lambda: eng.pool_backward(rows, w1, b1, w2.view(-1), scores, stats, pooled, dp, out=out, beta=0.5)) == N.E_INVALID
    assert all(float(o.abs().max()) == 0.0 for o in out)     # nothing was launched: the outputs are as they were
    odd = torch.zeros(63 * 256 + 1, device="cuda")[1:].view(1, 63, 256)                      # 4 bytes off a 16-byte boundary
    assert code(lambda: eng.pool_forward(odd, w1, b1, w2.view(-1), b2)) == N.E_INVALID
    assert code(lambda: eng.pool_backward(odd, w1, b1, w2.view(-1), scores, stats, pooled, dp)) == N.E_INVALID
    assert eng.chunk_reads_for(130) == 4 and eng.chunk_reads_for(32769) == 4
    with pytest.raises(ValueError):                          # a weight of the wrong size never reaches the kernel
        eng.pool_forward(rows, w1[:128], b1, w2.view(-1), b2)
