"""The predict loop that `lightning.Trainer.predict` runs in the reference
(/root/reference/chimeralm/__main__.py:307-317; call stack in SURVEY.md section 3.1), without Lightning:

    for batch in datamodule.predict_dataloader():      # collated on the host (pad-to-longest, file order)
        H2D copy on a side stream (pinned staging, overlapped with the previous batch's compute)
        logits, labels = model.predict_step(batch)      # MI355X engine
        writer.write_on_batch_end(...)                  # {rank}_{batch}.txt, "name<TAB>label"

Results leave the device one batch behind: the logits of batch i are copied to page-locked host memory right behind their
forward, the forward of batch i+1 is enqueued, and only then does the host wait for copy i and write its file -- the GPU never
idles while Python formats read names (the reference syncs on every batch, callbacks.py:107).

With an `attention_writer` (callbacks.AttentionWriter; `predict --save-attention`) every batch's attention summary, peaks and --
if asked for -- per-position weights (csrc/attn_weights.hip) take the same road: device -> page-locked host memory behind the forward,
read one batch behind, after the same event as the logits.  No wait is added per batch.

With a `trajectory_writer` (callbacks.TrajectoryWriter; `predict --save-trajectory`) every batch's running verdict -- the logits at
every multiple of the stride along each read and the per-read summary (csrc/trajectory.hip) -- takes that road as well.

`run_test` is the loop of `lightning.Trainer.test` over the same double buffer: `model.test_step(batch)` queues the batch's metric
update (csrc/eval_metrics.hip) behind its forward, so neither logits nor labels come back and the host waits for nothing per batch.

`run_explain` scans every read of every batch for the bases its prediction rests on (explain.position_importance: mutants built on
the device, the net's own forward, csrc/explain.hip) and hands the results to a `callbacks.ExplainWriter` one read behind.

`run_predict_native` is the same loop fed by the native BAM feeder (csrc/bam_feeder.cpp): a C++ thread decodes, selects,
tokenises and collates into a ring of page-locked slots; each batch crosses PCIe as uint8 on the engine's copy stream
(`clm_stage_ids`) while the previous batch is computing, and the slot goes back to the ring once its copy has landed.

With `long_reads` (a `longread.Options` of mode "tile"; `predict --long-reads tile`) both predict loops take UNTRUNCATED batches --
the data path is opened with `long_reads.max_tokens` -- which cross PCIe as uint8 on the copy stream and go through
`longread.tiled_forward`: the head batch is the batch the truncating path delivers, the extra windows of the long reads follow
through the same forward (and the same fp16c guard), and the reduced logits take the `_Deferred` road like any batch's.  A
`callbacks.WindowWriter` writes the per-window table behind the same event.  Without `long_reads` the loops run exactly as before.

With `batching` (a `bucket.Options` of mode "bucket"; `predict --batching bucket`) the staged device batches of either loop go through
`bucket.regroup` before `predict_step`: every read is padded to a canonical length of its own and reads of one such length are
forwarded together, so a read's logits no longer depend on its batch-mates; file `{rank}_{k}.txt` is the rank's k-th emitted batch.
Without `batching` the loops run exactly as before.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .distributed import LogitsGather


def _to_device(batch: dict, device: torch.device, stream: torch.cuda.Stream, device_keys: tuple = (), lengths=None) -> dict:
    """`lengths` (the long-read loop's `longread.Options`): the batch also carries its rows' token counts (host, found before the
    copy), and one that holds a long read lands in rows whose stride is a multiple of 16, as the window kernel reads them.  With
    the bucketed loop's `bucket.Options` every batch does: the scatter kernel reads them all."""
    out = {}
    with torch.cuda.stream(stream):
        for k, v in batch.items():
            if k == "input_ids" and lengths:
                from .longread import needs_windows, row_lengths

                u8 = v.to(torch.uint8)
                out["lengths"] = row_lengths(u8.numpy())
                if getattr(lengths, "mode", None) == "bucket" or needs_windows(out["lengths"], u8.shape[1], lengths):
                    host = torch.empty((u8.shape[0], (u8.shape[1] + 15) // 16 * 16), dtype=torch.uint8, pin_memory=True)
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

    With a `LogitsGather` the batch also takes part in the all-gather of this round: every rank contributes a
    `[rows, 3]` tensor (logit0, logit1, valid) -- short or empty batches are padded with valid = 0 -- on the gather's own stream,
    behind this forward only; the gathered `[world * rows, 3]` tensor follows to page-locked host memory on that stream."""

    def __init__(self, logits: torch.Tensor | None, labels, batch: dict | None, batch_idx: int,
                 gather: LogitsGather | None = None, rows: int = 0, device: torch.device | None = None, attention=None,
                 windows=None, window_writer=None, trajectory=None, trajectory_writer=None):
        self.host, self.event = None, None
        self.trajectory, self.trajectory_writer = None, trajectory_writer   # engine.TrajectoryOutput of host tensors, behind the same event
        self.attention = None                                  # engine.AttentionOutput of host tensors, behind the same event
        self.windows, self.window_writer = None, window_writer  # longread.TiledLogits of host tensors, behind the same event
        if logits is not None and logits.is_cuda:
            self.host = torch.empty(logits.shape, dtype=logits.dtype, pin_memory=True)   # caching host allocator: cheap after the first
            self.host.copy_(logits, non_blocking=True)
            if attention is not None:
                self.attention = attention.to_host()
            if windows is not None and window_writer is not None and windows.plan.n_extra:
                self.windows = windows.to_host()
            if trajectory is not None and trajectory_writer is not None:
                self.trajectory = trajectory.to_host()
            self.event = torch.cuda.Event()
            self.event.record()
        elif logits is not None:                               # host tensors: the CPU rehearsal of the multi-rank protocol (tests)
            self.host = logits
            self.attention = attention
            self.trajectory = trajectory if trajectory_writer is not None else None
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

    def flush(self, writer, trainer, model, on_batch, attention_writer=None) -> bool:
        """Write this batch's file; hand the gathered round to `on_batch`.  Returns whether ANY rank had reads in this round."""
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
            if attention_writer is not None and self.attention is not None:
                attention_writer.write_on_batch_end(trainer, model, (self.host, self.labels), self.attention, self.batch, self.batch_idx)
            if self.windows is not None:
                self.window_writer.write_on_batch_end(trainer, self.windows, self.batch, self.batch_idx)
            if self.trajectory is not None:
                self.trajectory_writer.write_on_batch_end(trainer, self.trajectory, self.batch, self.batch_idx)
        return alive


def _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch, attention_writer=None):
    """Ranks run out of reads at different times, but a collective needs every rank: a rank that is done keeps contributing
    empty rounds until one round has come back with no valid row from anybody.  All ranks see the same gathered tensors one
    round behind, so all of them leave this loop after the same number of rounds."""
    while True:
        now = _Deferred(None, None, None, batch_idx, gatherer, rows, device)
        alive = pending.flush(writer, trainer, model, on_batch, attention_writer) if pending is not None else True
        pending = now
        batch_idx += 1
        if not alive:
            break
    pending.flush(writer, trainer, model, on_batch, attention_writer)


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

    net = model.net
    if not isinstance(net, HyenaDna):
        raise ValueError(f"a trajectory needs a causal net: a prefix of a read must not know what follows it.  {type(net).__name__} is "
                         "not the Hyena net (the transformer attends in both directions, the CNN's windows straddle every cut; the "
                         "Mamba nets are causal and could follow, they are not built)")
    if long_reads is not None and getattr(long_reads, "mode", None) == "tile":
        raise ValueError("a read reduced from several windows has no single row to follow: no trajectory writer with long_reads")
    if net.trajectory_stride is None:
        raise ValueError("a trajectory writer needs a net built with trajectory_stride (HyenaDna(trajectory_stride=...))")
    return net.trajectory_request()


def _long_read_setup(long_reads, writer, attention_writer):
    """The options of a loop that tiles long reads (None: it does not) and the writer of its window tables, next to the predictions."""
    if long_reads is None or long_reads.mode != "tile":
        return None, None
    if attention_writer is not None:
        raise ValueError("the pooling weights of a read reduced from several windows are not defined: no attention writer with long_reads")
    from .callbacks import WindowWriter

    return long_reads, WindowWriter(writer.output_dir)


def _batching_setup(batching, long_reads, gather: bool, on_batch, pad_left: bool):
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
    return batching


def _run_predict_bucket(model, staged, writer, device: torch.device, rows: int, batching, *, rank: int, attention_writer,
                        trajectory_writer=None) -> int:
    """The predict loop over `bucket.regroup(staged)`: each emitted batch through `predict_step` (the module's own forward, so the
    16-bit guard hears every batch), its logits on the `_Deferred` road like any batch's."""
    import logging

    from .bucket import Regrouper, regroup

    model.eval()
    trainer = SimpleNamespace(global_rank=rank)
    n_reads, batch_idx = 0, 0
    pending: _Deferred | None = None
    want_attention = _attention_setup(model, attention_writer) is not None
    want_trajectory = _trajectory_setup(model, trajectory_writer) is not None
    regrouper = Regrouper(device, rows, batching)
    try:
        with torch.inference_mode():
            for cur in regroup(staged, regrouper):
                logits, labels = model.predict_step(cur, batch_idx)
                now = _Deferred(logits, labels, cur, batch_idx, attention=model.net.last_attention if want_attention else None,
                                trajectory=model.net.last_trajectory if want_trajectory else None, trajectory_writer=trajectory_writer)
                if pending is not None:
                    pending.flush(writer, trainer, model, None, attention_writer)
                pending = now
                n_reads += logits.shape[0]
                batch_idx += 1
            _check_engine(model, device, batch_idx)
            if pending is not None:
                pending.flush(writer, trainer, model, None, attention_writer)
    finally:
        regrouper.close()
    logging.getLogger(__name__).info("[rank %d] bucketed predict: %d reads in %d batches, %s tokens forwarded", rank, n_reads, batch_idx,
                                     f"{regrouper.n_tokens:,}")
    return n_reads


def run_predict(model, datamodule, writer, device: torch.device, *, rank: int = 0, gather: bool = False,
                on_batch=None, attention_writer=None, long_reads=None, batching=None, trajectory_writer=None) -> int:
    """Returns the number of reads this rank classified.  `gather`: every batch's logits are also all-gathered over the process
    group (RCCL over xGMI when the backend is "nccl"), off the compute stream, and handed to `on_batch(batch_idx, tensor)` one
    batch behind as a `[world * rows, 3]` host tensor (logit0, logit1, valid), rank r's rows at [r * rows, (r + 1) * rows).
    `long_reads`: see the module docstring; the datamodule must deliver untruncated reads (`max_length=long_reads.max_tokens`).
    `batching`: see the module docstring; the reads of this rank's shard are regrouped at the datamodule's per-device batch size."""
    want_trajectory = _trajectory_setup(model, trajectory_writer, long_reads) is not None
    batching = _batching_setup(batching, long_reads, gather, on_batch,
                               getattr(getattr(datamodule, "tokenizer", None), "padding_side", "left") == "left")
    if batching is not None:
        rows = getattr(datamodule, "batch_size_per_device", 0) or getattr(datamodule, "batch_size", 0)
        if not rows:
            raise ValueError("batching 'bucket' needs a datamodule that knows its batch size (batch_size_per_device)")
        return _run_predict_bucket(model, _staged_batches(datamodule.predict_dataloader(), device, lengths=batching), writer, device,
                                   int(rows), batching, rank=rank, attention_writer=attention_writer,
                                   trajectory_writer=trajectory_writer)
    long_reads, window_writer = _long_read_setup(long_reads, writer, attention_writer)
    if long_reads is not None:
        from .longread import tiled_forward

        if getattr(datamodule, "max_length", None) != long_reads.max_tokens:
            raise ValueError(f"long_reads needs a datamodule with max_length={long_reads.max_tokens} (max_bases and [SEP])")
    model.eval()
    trainer = SimpleNamespace(global_rank=rank)
    gatherer = LogitsGather(device) if gather else None
    rows = getattr(datamodule, "batch_size_per_device", 0)
    n_reads, batch_idx = 0, 0
    pending: _Deferred | None = None
    want_attention = _attention_setup(model, attention_writer) is not None
    with torch.inference_mode():
        for cur in _staged_batches(datamodule.predict_dataloader(), device, lengths=long_reads):
            tiled = None
            if long_reads is None:
                logits, labels = model.predict_step(cur, batch_idx)
            else:
                tiled = tiled_forward(model, cur["input_ids"], options=long_reads, batch_size=max(1, rows or cur["input_ids"].shape[0]),
                                      lengths=cur["lengths"])
                logits, labels = tiled.logits, cur["labels"]
            now = _Deferred(logits, labels, cur, batch_idx, gatherer, rows,
                            attention=model.net.last_attention if want_attention else None,   # (left by this batch's forward)
                            windows=tiled, window_writer=window_writer,
                            trajectory=model.net.last_trajectory if want_trajectory else None, trajectory_writer=trajectory_writer)
            if pending is not None:
                pending.flush(writer, trainer, model, on_batch, attention_writer)   # batch i-1: its copy finished while batch i was enqueued
            pending = now
            n_reads += logits.shape[0]
            batch_idx += 1
        _check_engine(model, device, batch_idx)
        if gatherer is not None:
            _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch, attention_writer)
        elif pending is not None:
            pending.flush(writer, trainer, model, on_batch, attention_writer)
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
    if eng is None:
        return
    from .engine import EngineError

    try:
        eng.check()
    except EngineError as e:
        raise EngineError(e.code, f"{e} [detected after batch {batch_idx - 1}, the last of this rank]") from None


def _run_predict_native_tiled(model, feeder, writer, window_writer, long_reads, device: torch.device, *, rank: int, gather: bool,
                              on_batch) -> int:
    """`run_predict_native` with `long_reads`: the untruncated slot crosses PCIe as uint8 on a copy stream, into rows whose stride
    is a multiple of 16, under the previous batch's forwards; the slot goes back to the ring after the copy's event; the batch goes
    through `longread.tiled_forward` (the module's own forward, so the 16-bit guard hears the head batch and the extra windows)."""
    import numpy as np

    from .longread import needs_windows, row_lengths, tiled_forward

    model.eval()
    trainer = SimpleNamespace(global_rank=rank)
    gatherer = LogitsGather(device) if gather else None
    rows = feeder.batch_size
    copy_stream = torch.cuda.Stream(device)
    compute = torch.cuda.current_stream(device)

    def stage(fb):
        host = np.lib.stride_tricks.as_strided(fb.ids, shape=(fb.n_reads, fb.n_tokens), strides=(fb.row_stride, 1))
        lengths = row_lengths(host)
        # a batch that is forwarded as it is crosses as one contiguous copy, as on the truncating path; one with a long read lands
        # in rows the window kernel can read (torch copies it across and re-strides it on the device)
        stride = (fb.n_tokens + 15) // 16 * 16 if needs_windows(lengths, fb.n_tokens, long_reads) else fb.n_tokens
        with torch.cuda.stream(copy_stream):
            dev = torch.empty((fb.n_reads, stride), dtype=torch.uint8, device=device)
            dev[:, : fb.n_tokens].copy_(torch.from_numpy(host), non_blocking=True)     # (the slot is page-locked: no host wait)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return dev, lengths, done

    n_reads, batch_idx = 0, 0
    pending: _Deferred | None = None
    cur = feeder.next()
    staged = stage(cur) if cur is not None else None
    with torch.inference_mode():
        while cur is not None:
            nxt = feeder.next()
            nxt_staged = stage(nxt) if nxt is not None else None      # H2D of batch i+1 overlaps the forwards of batch i
            dev, lengths, done = staged
            compute.wait_event(done)
            dev.record_stream(compute)                                # allocated on the copy stream, read by this stream's kernels
            tiled = tiled_forward(model, dev[:, : cur.n_tokens], options=long_reads, batch_size=rows, lengths=lengths)
            done.synchronize()                                        # the copy has left the slot ...
            feeder.release(cur)                                       # ... which goes back to the decoder
            labels = torch.full((cur.n_reads,), -1, dtype=torch.int64)
            batch = {"id": torch.from_numpy(cur.names), "labels": labels}
            now = _Deferred(tiled.logits, labels, batch, batch_idx, gatherer, rows, windows=tiled, window_writer=window_writer)
            if pending is not None:
                pending.flush(writer, trainer, model, on_batch)
            pending = now
            n_reads += cur.n_reads
            batch_idx += 1
            cur, staged = nxt, nxt_staged
        _check_engine(model, device, batch_idx)
        if gatherer is not None:
            _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch)
        elif pending is not None:
            pending.flush(writer, trainer, model, on_batch)
    return n_reads


def _native_staged(feeder, device: torch.device):
    """The feeder's batches as staged device batches for `bucket.regroup`: each slot crosses PCIe as uint8 on a copy stream, into
    rows whose stride is a multiple of 16, under the forwards of the batches before it, with its rows' token counts found on the host
    first; the slot goes back to the ring once its copy has landed and the batches it filled are queued."""
    import numpy as np

    from .longread import row_lengths

    copy_stream = torch.cuda.Stream(device)
    compute = torch.cuda.current_stream(device)

    def stage(fb):
        host = np.lib.stride_tricks.as_strided(fb.ids, shape=(fb.n_reads, fb.n_tokens), strides=(fb.row_stride, 1))
        lengths = row_lengths(host)
        with torch.cuda.stream(copy_stream):
            dev = torch.empty((fb.n_reads, (fb.n_tokens + 15) // 16 * 16), dtype=torch.uint8, device=device)
            dev[:, : fb.n_tokens].copy_(torch.from_numpy(host), non_blocking=True)     # (the slot is page-locked: no host wait)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return dev, lengths, done

    cur = feeder.next()
    staged = stage(cur) if cur is not None else None
    while cur is not None:
        nxt = feeder.next()
        nxt_staged = stage(nxt) if nxt is not None else None          # H2D of batch i+1 overlaps the forwards batch i fills
        dev, lengths, done = staged
        compute.wait_event(done)
        dev.record_stream(compute)                                    # allocated on the copy stream, read by this stream's kernels
        yield {"input_ids": dev[:, : cur.n_tokens], "id": torch.from_numpy(cur.names), "lengths": lengths,
               "labels": torch.full((cur.n_reads,), -1, dtype=torch.int64)}   # tokenizer.py:113: predict labels are all -1
        done.synchronize()                                            # the copy has left the slot ...
        feeder.release(cur)                                           # ... which goes back to the decoder
        cur, staged = nxt, nxt_staged


def run_predict_native(model, feeder, writer, device: torch.device, *, rank: int = 0, gather: bool = False,
                       on_batch=None, attention_writer=None, long_reads=None, batching=None, trajectory_writer=None) -> int:
    """Predict loop over a `chimeralm_amd.feeder.BamFeeder`; same files as `run_predict` over `BamDataModule`.  `long_reads`: see the
    module docstring; the feeder must be opened with `max_tokens=long_reads.max_tokens`.  `batching`: see the module docstring; the
    reads are regrouped at the feeder's batch size."""
    from ._native import DT_U8

    traj_request = _trajectory_setup(model, trajectory_writer, long_reads)
    batching = _batching_setup(batching, long_reads, gather, on_batch, getattr(feeder, "pad_left", True))
    if batching is not None:
        return _run_predict_bucket(model, _native_staged(feeder, device), writer, device, feeder.batch_size, batching, rank=rank,
                                   attention_writer=attention_writer, trajectory_writer=trajectory_writer)
    long_reads, window_writer = _long_read_setup(long_reads, writer, attention_writer)
    if long_reads is not None:
        return _run_predict_native_tiled(model, feeder, writer, window_writer, long_reads, device, rank=rank, gather=gather,
                                         on_batch=on_batch)

    model.eval()
    eng = model.net.engine(device)
    trainer = SimpleNamespace(global_rank=rank)
    gatherer = LogitsGather(device) if gather else None
    rows = feeder.batch_size
    n_reads, batch_idx = 0, 0
    pending: _Deferred | None = None
    request = _attention_setup(model, attention_writer)
    cur = feeder.next()
    staged = eng.stage_host_ids(cur.ids_ptr, DT_U8, cur.row_stride, cur.n_reads, cur.n_tokens) if cur is not None else -1
    with torch.inference_mode():
        while cur is not None:
            nxt = feeder.next()                               # already decoded by the feeder thread, normally
            nxt_staged = (eng.stage_host_ids(nxt.ids_ptr, DT_U8, nxt.row_stride, nxt.n_reads, nxt.n_tokens)
                          if nxt is not None else -1)         # H2D of batch i+1 overlaps the forward of batch i
            # the 16-bit mode against the exact-fp32 kernels on this batch's first reads, where a self-check is due (HyenaDna.guard)
            # (a callable: the host copy + H2D of the sampled rows happens only on the few batches a check is due for)
            model.net.guard(eng, lambda c=cur: torch.from_numpy(c.ids[: c.n_reads, : c.n_tokens][
                model.net._sample_rows(c.n_reads, model.net._BATCH_ROWS)].copy()).to(device), n_tokens=cur.n_tokens, n_reads=cur.n_reads)
            attention = trajectory = None
            if request is None and traj_request is None:
                logits = eng.forward_staged(staged, cur.n_reads)
            else:
                logits, *extra = eng.forward_staged(staged, cur.n_reads, attention=request, length=cur.n_tokens, trajectory=traj_request)
                trajectory = extra.pop() if traj_request is not None else None
                attention = extra[0] if request is not None else None
            eng.stage_wait(staged)                            # the copy has left the slot ...
            feeder.release(cur)                               # ... which goes back to the decoder
            labels = torch.full((cur.n_reads,), -1, dtype=torch.int64)   # tokenizer.py:113: predict labels are all -1
            batch = {"id": torch.from_numpy(cur.names), "labels": labels}
            now = _Deferred(logits, labels, batch, batch_idx, gatherer, rows, attention=attention, trajectory=trajectory,
                            trajectory_writer=trajectory_writer)
            if pending is not None:
                pending.flush(writer, trainer, model, on_batch, attention_writer)
            pending = now
            n_reads += cur.n_reads
            batch_idx += 1
            cur, staged = nxt, nxt_staged
        _check_engine(model, device, batch_idx)
        if gatherer is not None:
            _drain_gather(pending, gatherer, rows, device, batch_idx, writer, trainer, model, on_batch, attention_writer)
        elif pending is not None:
            pending.flush(writer, trainer, model, on_batch, attention_writer)
    return n_reads
