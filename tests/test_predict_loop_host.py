"""CPU: the one deferred-write loop of chimeralm_amd/predict.py (`_deferred_loop`) on host tensors, with recording stubs for what plugs
into it -- a source, a step, the writers, the engine -- in the style of tests/test_guard_logic.py.  What the loop computes on the device
is the GPU tests' business (tests/test_gpu_parity.py compares the files of both data paths); the ORDER of its calls is checked here."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from chimeralm_amd import predict as loop

DEVICE = torch.device("cpu")


class Recorder:
    """One event log shared by the stubs."""

    def __init__(self):
        self.log = []

    def writer(self):
        return SimpleNamespace(write_on_batch_end=lambda trainer, model, prediction, indices, batch, batch_idx, dl=0:
                               self.log.append(("write", batch_idx, tuple(prediction[0].shape), trainer.global_rank)))

    def model(self):
        """A module whose net holds an engine: `_check_engine` asks it once after the last batch."""
        return SimpleNamespace(net=SimpleNamespace(_engine=SimpleNamespace(check=lambda: self.log.append(("check",)))))


class Payload:
    def __init__(self, batch_idx):
        self.batch_idx = batch_idx

    def to_host(self):
        return self


def test_files_are_written_one_batch_behind_the_check_before_the_last_and_an_extra_after_its_prediction():
    rec = Recorder()
    source = [{"id": None, "labels": torch.full((n,), -1)} for n in (3, 3, 2)]

    def step(batch, batch_idx):
        rec.log.append(("step", batch_idx))
        write = lambda trainer, model, prediction, payload, b, idx: rec.log.append(("extra", idx, payload.batch_idx, b is batch))
        return torch.zeros((batch["labels"].shape[0], 2)), batch["labels"], [(Payload(batch_idx), write)]

    n = loop._deferred_loop(source, step, rec.writer(), rec.model(), DEVICE, rank=5)
    assert n == 8
    assert [e[:2] for e in rec.log] == [("step", 0), ("step", 1), ("write", 0), ("extra", 0), ("step", 2), ("write", 1), ("extra", 1),
                                        ("check",), ("write", 2), ("extra", 2)]
    assert [e[2:] for e in rec.log if e[0] == "write"] == [((3, 2), 5), ((3, 2), 5), ((2, 2), 5)]     # each batch's own logits; the rank
    assert [e[2:] for e in rec.log if e[0] == "extra"] == [(0, True), (1, True), (2, True)]           # each batch's own payload and dict


def test_an_empty_source_writes_nothing():
    rec = Recorder()
    assert loop._deferred_loop([], lambda batch, idx: 1 / 0, rec.writer(), rec.model(), DEVICE) == 0
    assert rec.log == [("check",)]


def test_extras_are_written_in_the_order_the_step_gives_them_and_none_is_skipped():
    rec = Recorder()
    mark = lambda name: (lambda trainer, model, prediction, payload, batch, idx: rec.log.append((name, idx)))

    def step(batch, batch_idx):
        return torch.zeros((1, 2)), batch["labels"], zip([Payload(0), None, Payload(0)], [mark("attention"), mark("windows"), mark("trajectory")])

    loop._deferred_loop([{"id": None, "labels": torch.full((1,), -1)}], step, rec.writer(), None, DEVICE)
    assert [e[0] for e in rec.log] == ["write", "attention", "trajectory"]


def test_the_direct_path_stages_ahead_and_releases_the_slot_before_anything_is_written():
    """`_engine_staged_batches` + `_direct_step` with a stub feeder and a stub engine: per batch -- stage i+1, guard, forward i, wait for
    copy i, release slot i, and only then the files of batch i-1."""
    rec = Recorder()
    sizes = [3, 3, 2]
    slots = [SimpleNamespace(slot=i, n_reads=n, n_tokens=7, row_stride=16, ids_ptr=1000 + i, ids=np.zeros((n, 16), np.uint8),
                             names=np.zeros((n, 256), np.int8)) for i, n in enumerate(sizes)]
    feeder = SimpleNamespace(next=lambda it=iter(slots): next(it, None), release=lambda fb: rec.log.append(("release", fb.slot)), batch_size=3)

    class Eng:
        def stage_host_ids(self, ptr, dtype, row_stride, n_reads, n_tokens):
            rec.log.append(("stage", ptr - 1000))
            return (ptr - 1000) % 2                                     # the engine's two staging buffers

        def forward_staged(self, staged, n_reads, **requests):
            rec.log.append(("forward", staged, n_reads, sorted(requests)))
            return torch.zeros((n_reads, 2))

        def stage_wait(self, staged):
            rec.log.append(("wait", staged))

        def check(self):
            rec.log.append(("check",))

    eng = Eng()
    net = SimpleNamespace(_engine=eng, guard=lambda e, ids, n_tokens, n_reads: rec.log.append(("guard", n_reads, callable(ids))))
    model = SimpleNamespace(net=net)
    run = SimpleNamespace(attention=None, trajectory=None, writes=[])
    n = loop._deferred_loop(loop._engine_staged_batches(feeder, eng), loop._direct_step(model, eng, run, DEVICE), rec.writer(), model, DEVICE)
    assert n == 8

    def batch(i):
        return [("guard", sizes[i], True), ("forward", i % 2, sizes[i], []), ("wait", i % 2), ("release", i)]

    assert [e[:2] if e[0] == "write" else e for e in rec.log] == (
        [("stage", 0), ("stage", 1)] + batch(0) + [("stage", 2)] + batch(1) + [("write", 0)] + batch(2) + [("write", 1), ("check",), ("write", 2)])


def test_a_feeder_slot_nobody_released_goes_back_when_the_next_batch_is_asked_for():
    """The bucketed run's consumer (`bucket.regroup`) never releases: the source does, once, when it is resumed."""
    rec = Recorder()
    slots = [SimpleNamespace(slot=i, n_reads=1, n_tokens=7, row_stride=16, ids_ptr=0, ids=None, names=np.zeros((1, 256), np.int8)) for i in range(2)]
    feeder = SimpleNamespace(next=lambda it=iter(slots): next(it, None), release=lambda fb: rec.log.append(("release", fb.slot)))
    eng = SimpleNamespace(stage_host_ids=lambda *a: 0, stage_wait=lambda staged: rec.log.append(("wait",)))
    for i, batch in enumerate(loop._engine_staged_batches(feeder, eng)):
        rec.log.append(("batch", i))
        if i == 0:
            loop._release(batch)                                         # the consumer got there first: not released twice
    assert rec.log == [("batch", 0), ("wait",), ("release", 0), ("batch", 1), ("wait",), ("release", 1)]
