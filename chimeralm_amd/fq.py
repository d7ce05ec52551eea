"""Parquet input of the test and predict stages, mirroring /root/reference/chimeralm/data/fq.py (`data: fq`, what the reference's
`eval.yaml` selects).

Same constructor (:63-79), `prepare_data` (:104-133), `setup` (:135-267) for the stages "test" and "predict" and
`test_dataloader` / `predict_dataloader` (:297-323).  A file has the columns `id`, `seq` (and `qual`, which no net reads); a
labelled read's id ends in `|0` or `|1` (tokenizer.parse_target).  The reference materialises HF `datasets` Arrow caches of the
whole file; here `pyarrow.parquet` streams it one row group at a time, so memory holds one row group and one batch whatever the
size of the file (same reads, same order, same batches).  There is no training path: `setup("fit")` raises.

With `world_size > 1` rank r takes reads r, r+G, r+2G, ... of the set, each read exactly once.  Lightning's distributed sampler
repeats reads from the start of the set to even out the ranks, which counts them twice in the metrics; this does not (DESIGN.md
section 3).
"""
from __future__ import annotations

from collections.abc import Iterator
from pathlib import Path

from .tokenizer import (ID_FEATURE, SEQ_FEATURE, DataCollator, tokenize_and_align_labels_and_quals,
                        tokenize_and_align_labels_and_quals_ids)

PARQUET_SUFFIX = ".parquet"


def percent_to_row(percent: int, num_rows: int) -> int:
    """The row a `train[{percent}%:]` split starts at: HF `datasets`' default rounding ("closest"), which is Python's `round`
    of the exact position (a tie goes to the even row)."""
    return int(round(percent * num_rows / 100.0))


def iter_rows(path: str | Path, start: int = 0, stop: int | None = None) -> Iterator[dict]:
    """`{"id", "seq"}` of rows [start, stop) in file order, one row group in memory at a time; row groups outside the range are
    not read."""
    import pyarrow.parquet as pq

    pf = pq.ParquetFile(str(path))
    stop = pf.metadata.num_rows if stop is None else min(stop, pf.metadata.num_rows)
    first = 0
    for g in range(pf.metadata.num_row_groups):
        n = pf.metadata.row_group(g).num_rows
        lo, hi = max(start, first), min(stop, first + n)
        if lo < hi:
            tab = pf.read_row_group(g, columns=[ID_FEATURE, SEQ_FEATURE])
            ids, seqs = tab.column(ID_FEATURE).to_pylist(), tab.column(SEQ_FEATURE).to_pylist()
            for i in range(lo - first, hi - first):
                yield {ID_FEATURE: ids[i], SEQ_FEATURE: seqs[i]}
        first += n
        if first >= stop:
            return


class DataModule:
    """Test- and predict-stage subset of the reference's LightningDataModule (same constructor arguments)."""

    def __init__(self, tokenizer, train_data_path=None, batch_size: int = 12, val_data_path=None, test_data_path=None,
                 predict_data_path=None, train_val_test_split=(0.7, 0.2, 0.1), num_workers: int = 0, max_train_samples=None,
                 max_val_samples=None, max_test_samples: int | None = None, max_predict_samples: int | None = None, *,
                 pin_memory: bool = False):
        self.tokenizer, self.batch_size = tokenizer, batch_size
        self.train_data_path, self.val_data_path = train_data_path, val_data_path
        self.test_data_path, self.predict_data_path = test_data_path, predict_data_path
        self.train_val_test_split = tuple(train_val_test_split)
        self.max_test_samples, self.max_predict_samples = max_test_samples, max_predict_samples
        self.num_workers, self.pin_memory = num_workers, pin_memory
        self.batch_size_per_device = batch_size
        self.data_collator = DataCollator(tokenizer)
        self.data_test: tuple[str, int, int] | None = None      # (file, first row, one past the last row)
        self.data_predict: tuple[str, int, int] | None = None
        self.world_size, self.rank = 1, 0

    @property
    def num_classes(self) -> int:
        return 2

    def prepare_data(self) -> None:
        for p in (self.train_data_path, self.val_data_path, self.test_data_path, self.predict_data_path):
            if p is not None and Path(p).suffix != PARQUET_SUFFIX:
                raise ValueError(f"Data file {p} is not in Parquet format.")

    @staticmethod
    def _num_rows(path) -> int:
        import pyarrow.parquet as pq

        if not Path(path).exists():
            raise FileNotFoundError(f"File not found: {path}")
        return pq.ParquetFile(str(path)).metadata.num_rows

    def setup(self, stage: str | None = None, world_size: int = 1, rank: int = 0) -> None:
        if stage not in ("test", "predict", None):
            raise NotImplementedError(f"stage {stage!r}: the MI355X engine has no training path; the parquet data module covers "
                                      "the test and predict stages")
        if self.batch_size % world_size != 0:
            raise RuntimeError(f"Batch size ({self.batch_size}) is not divisible by the number of devices ({world_size}).")
        self.world_size, self.rank = world_size, rank
        self.batch_size_per_device = self.batch_size // world_size
        self.prepare_data()
        if stage == "predict":
            if not self.predict_data_path:
                raise ValueError("Predict data path is required for prediction stage.")
            n = self._num_rows(self.predict_data_path)
            if self.max_predict_samples is not None:
                n = min(self.max_predict_samples, n)
            self.data_predict = (str(self.predict_data_path), 0, n)
            return
        if self.test_data_path is not None:
            # (the reference reads a test file only when a validation file comes with it, fq.py:195; a test stage has no use
            # for one, so a test file alone is enough here)
            path, first = self.test_data_path, 0
            last = self._num_rows(path)
        else:
            # fq.py:195-217: without a test file the three sets are percent slices of the training file, the test set its tail
            if not self.train_data_path:
                raise ValueError("the test stage needs data.test_data_path, or data.train_data_path to take the test tail from")
            path = self.train_data_path
            last = self._num_rows(path)
            a, b = int(100 * self.train_val_test_split[0]), int(100 * self.train_val_test_split[1])
            first = percent_to_row(a + b, last)
        if self.max_test_samples is not None:
            last = first + min(self.max_test_samples, last - first)
        self.data_test = (str(path), first, last)

    def _batches(self, rows: tuple[str, int, int], features) -> Iterator[dict]:
        max_length = self.tokenizer.max_len_single_sentence
        batch: list[dict] = []
        for i, rec in enumerate(iter_rows(*rows)):
            if self.world_size > 1 and i % self.world_size != self.rank:
                continue
            batch.append(features(rec, self.tokenizer, max_length))
            if len(batch) == self.batch_size_per_device:
                yield self.data_collator.torch_call(batch)
                batch = []
        if batch:
            yield self.data_collator.torch_call(batch)

    def test_dataloader(self) -> Iterator[dict]:
        """Batches of `input_ids` and `labels` in file order."""
        assert self.data_test is not None, "call setup('test') first"
        return self._batches(self.data_test, tokenize_and_align_labels_and_quals)

    def predict_dataloader(self) -> Iterator[dict]:
        """Batches of `input_ids`, `id` and `labels` (all -1) in file order."""
        assert self.data_predict is not None, "call setup('predict') first"
        return self._batches(self.data_predict, tokenize_and_align_labels_and_quals_ids)
