"""Host side of the one training loop (chimeralm_amd/fit.py, no GPU): the seeded order, the micro-batch shares, the best-epoch file,
and the two training steps against each other where both apply.  The head stub net and `_HostSums` live here; the stub fits of the
other nets (test_cnn_train_host.py, test_mamba_train_host.py) borrow `_HostSums`."""
from __future__ import annotations

from functools import partial
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import nn

REPO = Path(__file__).resolve().parent.parent
PARQUET = REPO / "tests" / "golden" / "tests.parquet"


class _Sin(nn.Module):
    def __init__(self):
        super().__init__()
        self.freq = nn.Parameter(torch.ones(1, 4))


class _StubBackbone(nn.Module):
    def __init__(self):
        super().__init__()
        act = _Sin()                                         # ONE module registered three times, as in the real filter
        self.implicit_filter = nn.Sequential(nn.Linear(2, 4), act, nn.Linear(4, 4), act, nn.Linear(4, 4), act)


class _StubHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.output_layer = nn.Linear(16, 2)


class _StubNet(nn.Module):
    """Logits from the base composition of a read, on CPU tensors."""

    def __init__(self, chunk_reads):
        super().__init__()
        self.number_of_classes, self.chunk_reads = 2, chunk_reads
        self.backbone, self.head = _StubBackbone(), _StubHead()
        for p in self.backbone.parameters():
            p.requires_grad = False
        self.seen = []

    def forward(self, ids, quals=None):
        if self.training:
            self.seen.append(ids.shape[0])
        counts = F.one_hot(ids, 16).double().mean(dim=1)
        return self.head.output_layer(counts)


class _HostSums:
    """EvalMetrics' sums for the stub's CPU logits (the fits' `metrics_factory`): same fields, same definitions."""

    def __init__(self):
        self.r = {"tp": 0, "fp": 0, "tn": 0, "fn": 0, "n_valid": 0, "n_batches": 0, "sum_batch_mean_loss": 0.0, "sum_loss": 0.0}

    def update(self, logits, labels):
        pred = logits.argmax(dim=-1)
        for k, (p, y) in (("tp", (1, 1)), ("fp", (1, 0)), ("tn", (0, 0)), ("fn", (0, 1))):
            self.r[k] += int(((pred == p) & (labels == y)).sum())
        loss = F.cross_entropy(logits.double(), labels, reduction="sum")
        self.r["n_valid"] += labels.numel()
        self.r["n_batches"] += 1
        self.r["sum_loss"] += float(loss)
        self.r["sum_batch_mean_loss"] += float(loss) / labels.numel()

    def read(self):
        return dict(self.r)

    def close(self):
        pass


def _stub_model(chunk_reads=2, seed=0):
    from chimeralm_amd.basic_module import ClassificationLit

    torch.manual_seed(seed)
    return ClassificationLit(net=_StubNet(chunk_reads).double(), optimizer=partial(torch.optim.AdamW, lr=1e-4, weight_decay=0.01),
                             scheduler=partial(torch.optim.lr_scheduler.ReduceLROnPlateau, mode="min", factor=0.1, patience=10))


def _fit(tmp, chunk_reads=2, seed=12345, epochs=2):
    from chimeralm_amd import headtrain

    model = _stub_model(chunk_reads)
    hist = headtrain.fit_head(model, (str(PARQUET), 0, 18), (str(PARQUET), 18, 25), tmp, epochs=epochs, batch_size=8, lr=1e-2,
                              seed=seed, device="cpu", metrics_factory=_HostSums)
    return model, hist


def test_epoch_order_is_a_function_of_seed_and_epoch():
    from chimeralm_amd.fit import epoch_order

    a = epoch_order(18, 12345, 0)
    assert sorted(a) == list(range(18))
    assert a == epoch_order(18, 12345, 0) and a != epoch_order(18, 12345, 1) and a != epoch_order(18, 12346, 0)
    torch.manual_seed(1)                                     # the global generator's state is not part of it
    assert a == epoch_order(18, 12345, 0)


def test_micro_losses_sum_to_the_batch_mean():
    from chimeralm_amd.fit import micro_loss

    g = torch.Generator().manual_seed(0)
    logits, labels = torch.randn(7, 2, generator=g, dtype=torch.float64), torch.tensor([0, 1, 1, 0, 1, 0, 0])
    total = sum(micro_loss(logits[b:b + 2], labels[b:b + 2], 7) for b in range(0, 7, 2))
    assert abs(float(total) - float(F.cross_entropy(logits, labels))) <= 1e-15


def test_best_epoch_file_round_trips(tmp_path):
    from safetensors.torch import load_file

    model, hist = _fit(tmp_path, epochs=1)
    saved = load_file(str(tmp_path / "model.safetensors"))
    own = model.state_dict()
    assert "net.backbone.implicit_filter.1.freq" in saved
    assert not [k for k in saved if k.endswith((".implicit_filter.3.freq", ".implicit_filter.5.freq"))]
    assert sorted(saved) == sorted(k for k in own if not k.endswith((".3.freq", ".5.freq")))
    fresh = _stub_model(seed=99)
    assert not torch.equal(fresh.net.head.output_layer.weight, model.net.head.output_layer.weight)
    fresh.load_reference_checkpoint(tmp_path / "model.safetensors")
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, own[k]), k


def test_the_two_steps_agree_where_both_apply(tmp_path):
    """On the head stub the backbone is frozen, so the head's parameters are all the trainable ones, and at chunk_reads = 16 a batch of
    8 is one micro-batch: the micro-batch step (sum / B of plain cross-entropy) and the whole-batch step (`model.criterion`, its
    mean) then state the same fit.  Every figure but `seconds` within 1e-12 -- the tolerance the micro-batch shares are held to
    against the whole batch in test_fit_head_on_a_stub_net -- and the saved tensors equal."""
    from safetensors.torch import load_file

    from chimeralm_amd import fit

    hists = {}
    for name, step in (("micro", fit.micro_batch_step), ("whole", fit.whole_batch_step)):
        model = _stub_model(chunk_reads=16)
        params = fit.trainable_parameters(model.net, "net")
        assert [id(p) for p in params] == [id(p) for p in model.net.head.parameters()]
        torch.manual_seed(12345)
        hists[name] = fit.fit(model, (str(PARQUET), 0, 18), (str(PARQUET), 18, 25), tmp_path / name, params=params, step=step, min_reads=1,
                              config="the stub", epochs=3, batch_size=8, lr=1e-2, seed=12345, device="cpu", metrics_factory=_HostSums)
        assert model.net.seen[:3] == [8, 8, 2]               # one forward per batch under either step
    assert len(hists["micro"]) == len(hists["whole"]) == 3
    for a, b in zip(hists["micro"], hists["whole"]):
        assert sorted(a) == sorted(b) == sorted(fit.METRIC_COLUMNS + ("val/f1_best",))
        for k in a:
            if k != "seconds":
                print(k, a[k], b[k])
                assert abs(a[k] - b[k]) <= 1e-12, (k, a[k], b[k])
    micro, whole = load_file(str(tmp_path / "micro" / "model.safetensors")), load_file(str(tmp_path / "whole" / "model.safetensors"))
    assert sorted(micro) == sorted(whole) and all(torch.equal(micro[k], whole[k]) for k in micro)
