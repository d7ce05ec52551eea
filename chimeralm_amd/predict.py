"""The predict loop that `lightning.Trainer.predict` runs in the reference
(/root/reference/chimeralm/__main__.py:307-317; call stack in SURVEY.md section 3.1), without Lightning:

    for batch in datamodule.predict_dataloader():      # collated on the host (pad-to-longest, file order)
        H2D copy on a side stream (pinned staging, overlapped with the previous batch's compute)
        logits, labels = model.predict_step(batch)      # MI355X engine
        writer.write_on_batch_end(...)                  # {rank}_{batch}.txt, "name<TAB>label"

ONE loop runs it for every data path and every option: `_deferred_loop(source, step, ...)`.  Results leave the device one batch
behind: the logits of batch i are copied to page-locked host memory right behind their forward (`_Deferred`), the forward of batch
i+1 is enqueued, and only then does the host wait for copy i and write its file -- the GPU never idles while Python formats read
names (the reference syncs on every batch, callbacks.py:107).  After the last batch the engine is asked once more (`_check_engine`)
before the last file is written; with gathered logits the ranks' rounds are drained (`_drain_gather`).  What plugs into the loop:

* a SOURCE, a generator of batch dicts with batch i+1 already staged when batch i is handed out:
  `_staged_batches` (a datamodule's loader: collated on the host, H2D on a copy stream), `_feeder_batches` (the native BAM feeder,
  csrc/bam_feeder.cpp: a C++ thread decodes, selects, tokenises and collates into a ring of page-locked slots; a slot crosses PCIe
  as uint8 on a copy stream, into rows of `_row_stride`), `_engine_staged_batches` (the feeder's slots on the ENGINE's copy stream,
  `clm_stage_ids`), or `bucket.regroup` around one of the first two.  A feeder batch carries `release`: the slot goes back to the
  ring once its copy has landed, as soon as the step has queued its work (`_release`) -- before anything is parked or written;
* a STEP, `step(batch, batch_idx) -> (logits, labels, extras)`: `_module_step` (`model.predict_step`), `_tiled_step`
  (`longread.tiled_forward`) or `_direct_step` (the fp16c guard, then `Engine.forward_staged`);
* EXTRAS, `(payload, write)` pairs of a step: a payload's `to_host()` copy rides to page-locked memory behind the logits, in front
  of the same event, and is written after the batch's prediction file.  No wait is added per batch.  Attention
  (callbacks.AttentionWriter, `predict --save-attention`: summary, peaks and -- if asked for -- per-position weights,
  csrc/attn_weights.hip), the window table of a tiled batch (callbacks.WindowWriter) and the running verdict
  (callbacks.TrajectoryWriter, `predict --save-trajectory`: the logits at every multiple of the stride along each read and the
  per-read summary, csrc/trajectory.hip) are the three there are, written in this order.

`run_predict` (a datamodule) and `run_predict_native` (a `feeder.BamFeeder`) resolve what the run asked for once (`_setup`: the
refusals, the requests, the writes), pick source and step, and call the loop.

With `long_reads` (a `longread.Options` of mode "tile"; `predict --long-reads tile`) both take UNTRUNCATED batches -- the data path
is opened with `long_reads.max_tokens` -- and the tiled step: the head batch is the batch the truncating path delivers, the extra
windows of the long reads follow through the same forward (and the same fp16c guard), and the reduced logits are the batch's.

With `batching` (a `bucket.Options` of mode "bucket"; `predict --batching bucket`) the staged device batches of either data path go
through `bucket.regroup` before the module step: every read is padded to a canonical length of its own and reads of one such length
are forwarded together, so a read's logits no longer depend on its batch-mates; file `{rank}_{k}.txt` is the rank's k-th emitted batch.

`run_test` is the loop of `lightning.Trainer.test` over `_staged_batches`: `model.test_step(batch)` queues the batch's metric
update (csrc/eval_metrics.hip) behind its forward, so neither logits nor labels come back and the host waits for nothing per batch.

`run_explain` scans every read of every batch for the bases its prediction rests on (explain.position_importance: mutants built on
the device, the net's own forward, csrc/explain.hip) and hands the results to a `callbacks.ExplainWriter` one read behind.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .distributed import LogitsGather


def _row_stride(options, lengths, n_tokens: int) -> int:
    """The stride of a batch's rows on the device, decided before it crosses PCIe.  A bucketed run's (`bucket.Options`) is always a
    multiple of 16: the scatter kernel reads every batch.  A tiling run's (`longread.Options`) is one only for a batch that holds a
    long read, as the window kernel reads it; any other is forwarded as it is and crosses as one contiguous copy, as on the
    truncating path."""
    from .longread import needs_windows

    padded = getattr(options, "mode", None) == "bucket" or needs_windows(lengths, n_tokens, options)
    return (n_tokens + 15) // 16 * 16 if padded else n_tokens


def _to_device(batch: dict, device: torch.device, stream: torch.cuda.Stream, device_keys: tuple = (), lengths=None) -> dict:
    """`lengths` (a tiling run's `longread.Options` or a bucketed run's `bucket.Options`): the batch also carries its rows' token
    counts (host, found before the copy) and lands in rows of `_row_stride`."""
    out = {}
    with torch.cuda.stream(stream):
        for k, v in batch.items():
            if k == "input_ids" and lengths:
                from .longread import row_lengths

                u8 = v.to(torch.uint8)
                out["lengths"] = row_lengths(u8.numpy())
                stride = _row_stride(lengths, out["lengths"], u8.shape[1])
                if stride != u8.shape[1]:
                    host = torch.empty((u8.shape[0], stride), dtype=torch.uint8, pin_memory=True)
                    host[:, : u8.shape[1]] = u8
                    v = host.to(device, non_blocking=True)[:, : u8.shape[1]]
                else:                                             # forwarded as it is: the truncating path's copy
                    v = u8.pin_memory().to(device, non_blocking=True)
            elif k == "input_ids":
                # ids fit a byte (vocabulary 12): 8x less PCIe traffic than the reference's int64 batch
                v = v.to(torch.uint8).pin_memory().to(device, non_blocking=True)
            elif k in device_keys:
                v = v.pin_memory().to(device, non_blocking=True)
            out[k] = v
    return out


def _staged_batches(loader, device: torch.device, device_keys: tuple = (), lengths=None):
    """The double buffer of the predict and test loops: yields batch i on the device once the compute stream waits for its copy,
    with batch i+1 already collated on the host and its H2D copy queued on a side stream -- under the forward the caller runs next."""
    copy_stream = torch.cuda.Stream(device)
    compute = torch.cuda.current_stream(device)
    it = iter(loader)
    nxt = next(it, None)
    staged = _to_device(nxt, device, copy_stream, device_keys, lengths) if nxt is not None else None
    while staged is not None:
        compute.wait_stream(copy_stream)
        cur = staged
        nxt = next(it, None)                              # host collation of batch i+1 ...
        staged = _to_device(nxt, device, copy_stream, device_keys, lengths) if nxt is not None else None   # ... and its H2D overlap
        for k, v in cur.items():
            if k == "input_ids" or k in device_keys:
                v.record_stream(compute)                  # allocated on the copy stream, read by the caller's kernels
        yield cur


class _Deferred:
    """The logits of one batch on their way to the host (async copy + event), and what the writer needs with them.

    `extras`: `(payload, write)` pairs -- attention, window tables, the trajectory, whatever a step hands over.  A payload's
    `to_host()` copy rides to page-locked memory behind the logits, in front of the same event, and `flush` calls
    `write(trainer, model, (logits, labels), payload, batch, batch_idx)` for each pair, in order, after the prediction file.

    With a `LogitsGather` the batch also takes part in the all-gather of this round: every rank contributes a
    `[rows, 3]` tensor (logit0, logit1, valid) -- short or empty batches are padded with valid = 0 -- on the gather's own stream,
    behind this forward only; the gathered `[world * rows, 3]` tensor follows to page-locked host memory on that stream."""

    def __init__(self, logits: torch.Tensor | None, labels, batch: dict | None, batch_idx: int,
                 gather: LogitsGather | None = None, rows: int = 0, device: torch.device | None = None, extras=()):
        self.host, self.event, self.extras = None, None, []
        if logits is not None and logits.is_cuda:
            self.host = torch.empty(logits.shape, dtype=logits.dtype, pin_memory=True)   # caching host allocator: cheap after the first
            self.host.copy_(logits, non_blocking=True)
            self.extras = [(payload.to_host(), write) for payload, write in extras if payload is not None]
            self.event = torch.cuda.Event()
            self.event.record()
        elif logits is not None:                               # host tensors: the CPU rehearsal of the protocol (tests)
            self.host, self.extras = logits, [(payload, write) for payload, write in extras if payload is not None]
        self.gathered, self.gathered_done = None, None
        if gather is not None:
            mine = torch.zeros((rows, 3), dtype=torch.float32, device=device if logits is None else logits.device)
            if logits is not None:
                mine[: logits.shape[0], :2] = logits
                mine[: logits.shape[0], 2] = 1.0
            full, done = gather.submit(mine)
            if done is not None:
                with torch.cuda.stream(gather.side):
                    self.gathered = torch.empty(full.shape, dtype=full.dtype, pin_memory=True)
                    self.gathered.copy_(full, non_blocking=True)
                    full.record_stream(gather.side)
                    self.gathered_done = torch.cuda.Event()
                    self.gathered_done.record(gather.side)
            else:
                self.gathered = full.cpu()
        self.labels, self.batch, self.batch_idx = labels, batch, batch_idx

    def flush(self, writer, trainer, model, on_batch) -> bool:
        """Write this batch's files; hand the gathered round to `on_batch`.  Returns whether ANY rank had reads in this round."""
        alive = self.host is not None
        if self.gathered is not None:
            if self.gathered_done is not None:
                self.gathered_done.synchronize()
            alive = bool((self.gathered[:, 2] > 0).any())
            if on_batch is not None and alive:
                on_batch(self.batch_idx, self.gathered)
        if self.host is not None:
            if self.event is not None:
                self.event.synchronize()
            writer.write_on_batch_end(trainer, model, (self.host, self.labels), None, self.batch, self.batch_idx, 0)
            for payload, write in self.extras:
                write(trainer, model, (self.host, self.labels), payload, self.batch, self.batch_idx)
        return alive


def _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch):
    """Ranks run out of reads at different times, but a collective needs every rank: a rank that is done keeps contributing
    empty rounds until one round has come back with no valid row from anybody.  All ranks see the same gathered tensors one
    round behind, so all of them leave this loop after the same number of rounds."""
    while True:
        now = _Deferred(None, None, None, batch_idx, gatherer, rows, device)
        alive = pending.flush(writer, trainer, model, on_batch) if pending is not None else True
        pending = now
        batch_idx += 1
        if not alive:
            break
    pending.flush(writer, trainer, model, on_batch)


def _deferred_loop(source, step, writer, model, device: torch.device, *, rank: int = 0, gatherer: LogitsGather | None = None,
                   rows: int = 0, on_batch=None) -> int:
    """THE predict loop, one batch behind: for every batch dict of `source`, `step(batch, batch_idx) -> (logits, labels, extras)`
    queues its forward, a `_Deferred` parks the outputs on their way to the host, and only then are the files of the batch BEFORE
    written -- its copies finished while this one was queued.  After the last batch the engine is asked once more, then the last
    file is written (with a `gatherer`: the rounds are drained).  Returns the number of reads.

    Nothing here touches the device: staging is the source's business, the forward the step's, the copies `_Deferred`'s -- on host
    tensors the loop runs as it is (tests/test_predict_loop_host.py)."""
    trainer = SimpleNamespace(global_rank=rank)
    n_reads, batch_idx = 0, 0
    pending: _Deferred | None = None
    with torch.inference_mode():
        for cur in source:
            logits, labels, extras = step(cur, batch_idx)
            now = _Deferred(logits, labels, cur, batch_idx, gatherer, rows, extras=extras)
            if pending is not None:
                pending.flush(writer, trainer, model, on_batch)    # batch i-1: its copy finished while batch i was enqueued
            pending = now
            n_reads += logits.shape[0]
            batch_idx += 1
        _check_engine(model, device, batch_idx)
        if gatherer is not None:
            _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch)
        elif pending is not None:
            pending.flush(writer, trainer, model, on_batch)
    return n_reads


# ------------------------------------------------------------------------------------------------ what a run asked for
def _attention_setup(model, attention_writer):
    """The net's attention request for a loop that writes attention files (None without a writer): the writer decides whether the
    per-position weights come along (`attention_writer.weights`)."""
    if attention_writer is None:
        return None
    net = model.net
    if getattr(net, "attention_top_k", None) is None:
        raise ValueError("an attention writer needs a net built with attention_top_k (HyenaDna(attention_top_k=...))")
    net.attention_device_weights = bool(getattr(attention_writer, "weights", False))
    return net.attention_request()


def _trajectory_setup(model, trajectory_writer, long_reads=None):
    """The net's trajectory request for a loop that writes trajectory files (None without a writer), after the refusals."""
    if trajectory_writer is None:
        return None
    from .hyena import HyenaDna
    from .mamba import MambaSequenceClassification, MambaSequenceClassificationSP

    net = model.net
    if not isinstance(net, (HyenaDna, MambaSequenceClassification, MambaSequenceClassificationSP)):
        raise ValueError(f"a trajectory needs a causal net: a prefix of a read must not know what follows it.  {type(net).__name__} is "
                         "neither the Hyena net nor one of the two Mamba nets (the transformer attends in both directions, the CNN's "
                         "windows and pools straddle every cut)")
    if long_reads is not None and getattr(long_reads, "mode", None) == "tile":
        raise ValueError("a read reduced from several windows has no single row to follow: no trajectory writer with long_reads")
    if net.trajectory_stride is None:
        raise ValueError(f"a trajectory writer needs a net built with trajectory_stride ({type(net).__name__}(trajectory_stride=...))")
    return net.trajectory_request()


def _long_read_setup(long_reads, writer, attention_writer):
    """The options of a loop that tiles long reads (None: it does not) and the writer of its window tables, next to the predictions."""
    if long_reads is None or long_reads.mode != "tile":
        return None, None
    if attention_writer is not None:
        raise ValueError("the pooling weights of a read reduced from several windows are not defined: no attention writer with long_reads")
    from .callbacks import WindowWriter

    return long_reads, WindowWriter(writer.output_dir)


def _batching_setup(batching, long_reads, gather: bool, on_batch, pad_left: bool, rows: int):
    """The options of a loop that regroups its reads by canonical length (None: it does not), after the refusals."""
    if batching is None or batching.mode != "bucket":
        return None
    if long_reads is not None and long_reads.mode == "tile":
        raise ValueError("batching 'bucket' and long_reads 'tile' exclude each other: a window plan is made per file-order batch")
    if gather or on_batch is not None:
        raise ValueError("batching 'bucket' and gathered logits exclude each other: logits.tsv identifies a read by its position in a "
                         "file-order batch, which a regrouped batch does not have")
    if not pad_left:
        raise ValueError("batching 'bucket' takes batches padded on the left only")
    if not rows:
        raise ValueError("batching 'bucket' needs a datamodule that knows its batch size (batch_size_per_device)")
    return batching


def _setup(model, writer, *, attention_writer, long_reads, batching, trajectory_writer, gather: bool, on_batch, pad_left: bool, rows: int):
    """What a run asked for, resolved once before its loop, the refusals in their order: the requests the forwards make (`attention`,
    `trajectory`), the options of a bucketed (`batching`) or tiling (`long_reads`) run, or None for each; `writes`, the `_Deferred`
    write of every request made, attention's before the trajectory's; `write_windows`, that of a tiling run's window tables."""
    def payload_only(w):                                      # (these writers take neither the module nor the prediction)
        return lambda trainer, pl_module, prediction, payload, batch, batch_idx: w.write_on_batch_end(trainer, payload, batch, batch_idx)

    run = SimpleNamespace(trajectory=_trajectory_setup(model, trajectory_writer, long_reads),
                          batching=_batching_setup(batching, long_reads, gather, on_batch, pad_left, rows))
    run.long_reads, window_writer = _long_read_setup(long_reads, writer, attention_writer)
    run.attention = _attention_setup(model, attention_writer)
    run.write_windows = payload_only(window_writer) if window_writer is not None else None
    run.writes = ([attention_writer.write_on_batch_end] if run.attention is not None else []) \
        + ([payload_only(trajectory_writer)] if run.trajectory is not None else [])
    return run


# ------------------------------------------------------------------------------------------------ steps: step(batch, batch_idx)
def _release(batch: dict) -> None:
    """Hands back the feeder slot a batch came in, where it has one that is still out (the feeder sources below)."""
    release = batch.pop("release", None)
    if release is not None:
        release()


def _module_step(model, run):
    """`model.predict_step`: the module's own forward (so the 16-bit guard hears every batch), which leaves what the run asked for
    in `net.last_attention` / `net.last_trajectory`."""
    def step(batch, batch_idx):
        logits, labels = model.predict_step(batch, batch_idx)
        got = ([model.net.last_attention] if run.attention is not None else []) \
            + ([model.net.last_trajectory] if run.trajectory is not None else [])
        return logits, labels, zip(got, run.writes)
    return step


def _tiled_step(model, run, rows: int):
    """`longread.tiled_forward` of an untruncated batch: the module's own forward for the head batch and, in chunks of `rows`, the
    extra windows; the reduced logits are the batch's, the window table goes along when the batch holds a long read.  A feeder
    slot goes back once the copy has left it, before anything is parked or written."""
    from .longread import tiled_forward

    def step(batch, batch_idx):
        ids = batch["input_ids"]
        tiled = tiled_forward(model, ids, options=run.long_reads, batch_size=max(1, rows or ids.shape[0]), lengths=batch["lengths"])
        _release(batch)
        return tiled.logits, batch["labels"], [(tiled, run.write_windows)] if tiled.plan.n_extra else []
    return step


def _direct_step(model, eng, run, device: torch.device):
    """The engine driven directly on a batch of `_engine_staged_batches`: the guard, `forward_staged`, and the slot goes back."""
    net = model.net

    def step(batch, batch_idx):
        fb = batch["slot"]
        # the 16-bit mode against the exact-fp32 kernels on this batch's first reads, where a self-check is due (HyenaDna.guard)
        # (a callable: the host copy + H2D of the sampled rows happens only on the few batches a check is due for)
        net.guard(eng, lambda: torch.from_numpy(fb.ids[: fb.n_reads, : fb.n_tokens][
            net._sample_rows(fb.n_reads, net._BATCH_ROWS)].copy()).to(device), n_tokens=fb.n_tokens, n_reads=fb.n_reads)
        if run.writes:
            logits, *got = eng.forward_staged(batch["staged"], fb.n_reads, attention=run.attention, length=fb.n_tokens,
                                              trajectory=run.trajectory)
        else:
            logits, got = eng.forward_staged(batch["staged"], fb.n_reads), []
        _release(batch)
        return logits, batch["labels"], zip(got, run.writes)
    return step


# ------------------------------------------------------------------------------------------------ the public loops
def run_predict(model, datamodule, writer, device: torch.device, *, rank: int = 0, gather: bool = False,
                on_batch=None, attention_writer=None, long_reads=None, batching=None, trajectory_writer=None) -> int:
    """Returns the number of reads this rank classified.  `gather`: every batch's logits are also all-gathered over the process
    group (RCCL over xGMI when the backend is "nccl"), off the compute stream, and handed to `on_batch(batch_idx, tensor)` one
    batch behind as a `[world * rows, 3]` host tensor (logit0, logit1, valid), rank r's rows at [r * rows, (r + 1) * rows).
    `long_reads`: see the module docstring; the datamodule must deliver untruncated reads (`max_length=long_reads.max_tokens`).
    `batching`: see the module docstring; the reads of this rank's shard are regrouped at the datamodule's per-device batch size."""
    rows = getattr(datamodule, "batch_size_per_device", 0)
    bucket_rows = int(rows or getattr(datamodule, "batch_size", 0))
    run = _setup(model, writer, attention_writer=attention_writer, long_reads=long_reads, batching=batching,
                 trajectory_writer=trajectory_writer, gather=gather, on_batch=on_batch, rows=bucket_rows,
                 pad_left=getattr(getattr(datamodule, "tokenizer", None), "padding_side", "left") == "left")
    if run.long_reads is not None and getattr(datamodule, "max_length", None) != run.long_reads.max_tokens:
        raise ValueError(f"long_reads needs a datamodule with max_length={run.long_reads.max_tokens} (max_bases and [SEP])")
    model.eval()
    staged = _staged_batches(datamodule.predict_dataloader(), device, lengths=run.batching or run.long_reads)
    if run.batching is not None:
        return _bucketed(model, staged, writer, device, bucket_rows, run, rank)
    step = _module_step(model, run) if run.long_reads is None else _tiled_step(model, run, rows)
    return _deferred_loop(staged, step, writer, model, device, rank=rank, gatherer=LogitsGather(device) if gather else None, rows=rows,
                          on_batch=on_batch)


def _bucketed(model, staged, writer, device: torch.device, rows: int, run, rank: int) -> int:
    """The loop over `bucket.regroup(staged)`: each emitted batch through the module step, and the run's one log line."""
    import logging

    from .bucket import Regrouper, regroup

    regrouper = Regrouper(device, rows, run.batching)
    try:
        n_reads = _deferred_loop(regroup(staged, regrouper), _module_step(model, run), writer, model, device, rank=rank)
    finally:
        regrouper.close()
    logging.getLogger(__name__).info("[rank %d] bucketed predict: %d reads in %d batches, %s tokens forwarded", rank, n_reads,
                                     regrouper.n_batches, f"{regrouper.n_tokens:,}")
    return n_reads


def run_test(model, datamodule, device: torch.device) -> int:
    """The test loop: every batch's forward and, behind it on the same stream, its metric update (`model.test_step`); no logits
    leave the device and nothing waits per batch.  Returns the number of reads this rank ran; the sums stay in
    `model.test_metrics` for the caller's one read."""
    model.eval()
    n_reads, batch_idx = 0, 0
    with torch.inference_mode():
        for cur in _staged_batches(datamodule.test_dataloader(), device, device_keys=("labels",)):
            model.test_step(cur, batch_idx)
            n_reads += cur["labels"].shape[0]
            batch_idx += 1
        _check_engine(model, device, batch_idx)
    return n_reads


def run_explain(model, datamodule, writer, device: torch.device, *, rank: int = 0, max_reads: int | None = None,
                batch_size: int = 256, **options) -> int:
    """Every read of every predict batch, stripped of the collator's left pads, through `explain.position_importance` (`options`:
    window, stride, substitute, score, top_k); `batch_size` is the number of mutants per forward.  A read's result follows to
    page-locked host memory behind its last kernel and is written while the next read's scan is queued.  A read the scan does not
    take (no base, or a token that is not A, C, G, T or N) is logged and left out.  Returns the number of reads written."""
    import logging

    from .callbacks import _read_names
    from .explain import Options, position_importance
    from .tokenizer import PAD_ID

    Options(**options)                                        # a bad option fails before the first read
    log = logging.getLogger(__name__)
    model.eval()
    trainer = SimpleNamespace(global_rank=rank)
    n_written, index = 0, 0
    pending = None                                            # (name, index, host Importance, event)

    def flush(p):
        p[3].synchronize()
        writer.write_read(trainer, p[0], p[1], p[2])

    with torch.cuda.device(device), torch.inference_mode():
        for batch in datamodule.predict_dataloader():
            if max_reads is not None and index >= max_reads:
                break
            names = _read_names(batch["id"])
            for row, name in zip(batch["input_ids"], names):
                if max_reads is not None and index >= max_reads:
                    break
                keep = (row != PAD_ID).nonzero()
                ids = row[int(keep[0]):] if keep.numel() else row[:0]
                try:
                    imp = position_importance(model, ids, batch_size=batch_size, device=device, **options)
                except ValueError as e:
                    log.warning("read %s is not scanned: %s", name, e)
                    index += 1
                    continue
                host = imp.to_host()
                done = torch.cuda.Event()
                done.record()
                if pending is not None:
                    flush(pending)
                pending = (name, index, host, done)
                index += 1
                n_written += 1
        if pending is not None:
            flush(pending)
    return n_written


def _check_engine(model, device: torch.device, batch_idx: int) -> None:
    """Errors only the device sees (token ids outside the embedding table: the reference raises IndexError inside the forward,
    hyena.py:249) are reported by the NEXT engine call -- after the last batch there is none, so ask once more before its file
    is written.  The message names the batch range it can belong to."""
    net = getattr(model, "net", None)
    eng = getattr(net, "_engine", None)
    if eng is None or not hasattr(eng, "check"):           # (SequenceCNNTransformer._engine is a method: its calls report their own errors)
        return
    from .engine import EngineError

    try:
        eng.check()
    except EngineError as e:
        raise EngineError(e.code, f"{e} [detected after batch {batch_idx - 1}, the last of this rank]") from None


def _feeder_batches(feeder, device: torch.device, options):
    """The feeder's batches as staged device batches, for a tiling or bucketed run (`options`): each slot crosses PCIe as uint8 on a
    copy stream, into rows of `_row_stride`, under the forwards of the batch before it, with its rows' token counts found on the host
    first.  The slot goes back to the ring once its copy has landed: when the consumer says its work is queued (`_release`), at the
    latest when it asks for the next batch."""
    import numpy as np

    from .longread import row_lengths

    copy_stream = torch.cuda.Stream(device)
    compute = torch.cuda.current_stream(device)

    def stage(fb):
        host = np.lib.stride_tricks.as_strided(fb.ids, shape=(fb.n_reads, fb.n_tokens), strides=(fb.row_stride, 1))
        lengths = row_lengths(host)
        with torch.cuda.stream(copy_stream):
            dev = torch.empty((fb.n_reads, _row_stride(options, lengths, fb.n_tokens)), dtype=torch.uint8, device=device)
            dev[:, : fb.n_tokens].copy_(torch.from_numpy(host), non_blocking=True)     # (the slot is page-locked: no host wait)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return dev, lengths, done

    def release(fb, done):
        done.synchronize()                                            # the copy has left the slot ...
        feeder.release(fb)                                            # ... which goes back to the decoder

    cur = feeder.next()
    staged = stage(cur) if cur is not None else None
    while cur is not None:
        nxt = feeder.next()
        nxt_staged = stage(nxt) if nxt is not None else None          # H2D of batch i+1 overlaps the forwards of batch i
        dev, lengths, done = staged
        compute.wait_event(done)
        dev.record_stream(compute)                                    # allocated on the copy stream, read by this stream's kernels
        batch = {"input_ids": dev[:, : cur.n_tokens], "id": torch.from_numpy(cur.names), "lengths": lengths,
                 "labels": torch.full((cur.n_reads,), -1, dtype=torch.int64),   # tokenizer.py:113: predict labels are all -1
                 "release": lambda fb=cur, done=done: release(fb, done)}
        yield batch
        _release(batch)
        cur, staged = nxt, nxt_staged


def _engine_staged_batches(feeder, eng):
    """The feeder's batches for `_direct_step`: each slot crosses PCIe as uint8 on the ENGINE's copy stream (`clm_stage_ids`), batch
    i+1 before batch i is handed out, so under its forward; `release` waits for the copy and hands the slot back."""
    from ._native import DT_U8

    def stage(fb):
        return eng.stage_host_ids(fb.ids_ptr, DT_U8, fb.row_stride, fb.n_reads, fb.n_tokens) if fb is not None else -1

    def release(fb, staged):
        eng.stage_wait(staged)                                        # the copy has left the slot ...
        feeder.release(fb)                                            # ... which goes back to the decoder

    cur = feeder.next()
    staged = stage(cur)
    while cur is not None:
        nxt = feeder.next()                                           # already decoded by the feeder thread, normally
        nxt_staged = stage(nxt)                                       # H2D of batch i+1 overlaps the forward of batch i
        batch = {"id": torch.from_numpy(cur.names), "labels": torch.full((cur.n_reads,), -1, dtype=torch.int64), "slot": cur,
                 "staged": staged, "release": lambda fb=cur, staged=staged: release(fb, staged)}
        yield batch
        _release(batch)
        cur, staged = nxt, nxt_staged


def run_predict_native(model, feeder, writer, device: torch.device, *, rank: int = 0, gather: bool = False,
                       on_batch=None, attention_writer=None, long_reads=None, batching=None, trajectory_writer=None) -> int:
    """Predict loop over a `chimeralm_amd.feeder.BamFeeder`; same files as `run_predict` over `BamDataModule`.  `long_reads`: see the
    module docstring; the feeder must be opened with `max_tokens=long_reads.max_tokens`.  `batching`: see the module docstring; the
    reads are regrouped at the feeder's batch size."""
    rows = getattr(feeder, "batch_size", 0)
    run = _setup(model, writer, attention_writer=attention_writer, long_reads=long_reads, batching=batching,
                 trajectory_writer=trajectory_writer, gather=gather, on_batch=on_batch, rows=rows, pad_left=getattr(feeder, "pad_left", True))
    model.eval()
    if run.batching is not None:
        return _bucketed(model, _feeder_batches(feeder, device, run.batching), writer, device, rows, run, rank)
    if run.long_reads is not None:
        source, step = _feeder_batches(feeder, device, run.long_reads), _tiled_step(model, run, rows)
    else:
        eng = model.net.engine(device)
        source, step = _engine_staged_batches(feeder, eng), _direct_step(model, eng, run, device)
    return _deferred_loop(source, step, writer, model, device, rank=rank, gatherer=LogitsGather(device) if gather else None, rows=rows,
                          on_batch=on_batch)
