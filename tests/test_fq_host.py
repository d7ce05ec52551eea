"""The parquet data module without a GPU: labels, the test tail's boundary and the first batch against
tests/golden/eval_golden.json (the reference's `parse_target`, HF `datasets`' own percent rounding, the reference's collator),
sharding, streaming over row groups, and what it refuses."""
from __future__ import annotations

import json
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gold(golden_dir):
    return json.loads((golden_dir / "eval_golden.json").read_text())["parquet"]


def _rows(path):
    import pyarrow.parquet as pq

    return pq.read_table(path).to_pylist()


def test_labels_equal_the_reference_parse_target(golden_dir, gold):
    from chimeralm_amd import tokenizer as T

    rows = _rows(golden_dir / "tests.parquet")
    assert len(rows) == gold["num_rows"] == 25
    assert [T.parse_target(r["id"])[1] for r in rows] == gold["labels"]
    assert sorted(set(gold["labels"])) == [0, 1]
    assert T.parse_target("a-read-without-a-label") == ("a-read-without-a-label", -1)
    assert T.parse_target("r|1") == ("r", 1)
    tok = T.CharTokenizer(model_max_length=100, add_cls=True)
    f = T.tokenize_and_align_labels_and_quals({"id": "r|0", "seq": "ACGT"}, tok, 98)
    assert f == {"input_ids": [0, 7, 8, 9, 10, 1], "labels": 0}
    with pytest.raises(NotImplementedError):
        T.tokenize_and_align_labels_and_quals({"id": "r|0", "seq": "ACGT"}, tok, 98, include_qual=True)


def test_test_tail_starts_where_the_datasets_library_starts_it(golden_dir, gold):
    from chimeralm_amd import fq, tokenizer as T

    tok = T.CharTokenizer(model_max_length=100, padding_side="left", add_cls=True)
    dm = fq.DataModule(tok, train_data_path=golden_dir / "tests.parquet", batch_size=12)
    dm.prepare_data()
    dm.setup("test")
    _, first, stop = dm.data_test
    assert (first, stop - 1) == (gold["tail_first_row"], gold["tail_last_row"])
    batches = list(dm.test_dataloader())
    assert len(batches) == 1 and set(batches[0]) == {"input_ids", "labels"}
    assert batches[0]["labels"].tolist() == gold["labels"][first:stop]
    dm.setup(None)                                             # Lightning's "all stages": the test set again
    assert dm.data_test == (str(golden_dir / "tests.parquet"), first, stop)
    # the rounding itself: a tie goes to the even row, as Python's round in the library
    assert [fq.percent_to_row(90, n) for n in (25, 15, 10, 1000, 7)] == [22, 14, 9, 900, 6]
    dm = fq.DataModule(tok, train_data_path=golden_dir / "tests.parquet", batch_size=12, max_test_samples=2)
    dm.setup("test")
    assert dm.data_test[1:] == (first, first + 2)


def test_first_batch_of_the_whole_file_has_the_reference_shape(golden_dir, gold):
    from chimeralm_amd import fq, tokenizer as T

    fb = gold["first_batch"]
    tok = T.CharTokenizer(model_max_length=fb["model_max_length"], padding_side=fb["padding_side"], add_cls=True)
    dm = fq.DataModule(tok, golden_dir / "tests.parquet", fb["batch_size"], test_data_path=golden_dir / "tests.parquet")
    dm.setup("test")
    batches = list(dm.test_dataloader())
    assert [b["input_ids"].shape[0] for b in batches] == [12, 12, 1]
    assert list(batches[0]["input_ids"].shape) == fb["input_ids_shape"] and batches[0]["input_ids"].dtype == torch.int64
    assert batches[0]["labels"].tolist() == fb["labels"] and batches[0]["labels"].dtype == torch.int64
    assert torch.cat([b["labels"] for b in batches]).tolist() == gold["labels"]


def test_two_ranks_see_every_row_exactly_once(golden_dir, gold):
    from chimeralm_amd import fq, tokenizer as T

    tok = T.CharTokenizer(model_max_length=2000, padding_side="left")
    rows = _rows(golden_dir / "tests.parquet")
    seen = []
    for rank in (0, 1):
        dm = fq.DataModule(tok, test_data_path=golden_dir / "tests.parquet", batch_size=12)
        dm.setup("test", world_size=2, rank=rank)
        assert dm.batch_size_per_device == 6
        mine = list(range(rank, 25, 2))
        got = list(dm.test_dataloader())
        assert [b["labels"].shape[0] for b in got] == ([6, 6, 1] if rank == 0 else [6, 6])
        assert torch.cat([b["labels"] for b in got]).tolist() == [gold["labels"][i] for i in mine]
        # a read's own tokens are the end of its left-padded row: tell rows apart by them
        for b, chunk in zip(got, (mine[0:6], mine[6:12], mine[12:])):
            for row, i in zip(b["input_ids"], chunk):
                want = tok.encode_array(rows[i]["seq"], tok.max_len_single_sentence)
                assert row[-len(want):].tolist() == want.tolist()
        seen += mine
    assert sorted(seen) == list(range(25))
    with pytest.raises(RuntimeError, match="not divisible"):
        fq.DataModule(tok, test_data_path=golden_dir / "tests.parquet", batch_size=12).setup("test", world_size=5, rank=0)


def test_several_row_groups_give_the_same_batches(golden_dir, tmp_path):
    import pyarrow.parquet as pq

    from chimeralm_amd import fq, tokenizer as T

    src = golden_dir / "tests.parquet"
    assert pq.ParquetFile(src).metadata.num_row_groups == 1
    small = tmp_path / "groups.parquet"
    pq.write_table(pq.read_table(src), small, row_group_size=4)
    assert pq.ParquetFile(small).metadata.num_row_groups == 7
    tok = T.CharTokenizer(model_max_length=2000, padding_side="left")
    for kw in ({"test_data_path": None}, {"max_test_samples": 2}, {}):
        for stage in ("test", "predict"):
            got = []
            for path in (src, small):
                args = dict(train_data_path=path, test_data_path=path, predict_data_path=path, batch_size=12, max_predict_samples=9)
                dm = fq.DataModule(tok, **{**args, **kw})
                dm.setup(stage, world_size=2, rank=1)
                got.append(list(dm.test_dataloader() if stage == "test" else dm.predict_dataloader()))
            assert len(got[0]) == len(got[1]) >= 1
            for a, b in zip(*got):
                assert set(a) == set(b) == ({"input_ids", "labels"} if stage == "test" else {"input_ids", "labels", "id"})
                assert all(torch.equal(a[k], b[k]) for k in a)
    assert [r["id"] for r in fq.iter_rows(small, 3, 9)] == [r["id"] for r in _rows(src)[3:9]]


def test_predict_stage_keeps_names_and_unknown_labels(golden_dir):
    from chimeralm_amd import fq, tokenizer as T
    from chimeralm_amd.callbacks import resume_read_name

    tok = T.CharTokenizer(model_max_length=2000, padding_side="left")
    dm = fq.DataModule(tok, predict_data_path=golden_dir / "tests.parquet", batch_size=12, max_predict_samples=5)
    with pytest.raises(AssertionError):
        dm.predict_dataloader()
    dm.setup("predict")
    (b,) = list(dm.predict_dataloader())
    assert b["input_ids"].shape[0] == 5 and b["labels"].tolist() == [-1] * 5
    assert [resume_read_name(r) for r in b["id"]] == [r["id"] for r in _rows(golden_dir / "tests.parquet")[:5]]
    with pytest.raises(ValueError, match="Predict data path"):
        fq.DataModule(tok, batch_size=12).setup("predict")


def test_what_it_refuses(golden_dir, tmp_path):
    from chimeralm_amd import bam, fq, tokenizer as T

    tok = T.CharTokenizer(model_max_length=100)
    with pytest.raises(ValueError, match="is not in Parquet format"):
        fq.DataModule(tok, test_data_path=tmp_path / "reads.fastq", batch_size=12).prepare_data()
    with pytest.raises(ValueError, match="is not in Parquet format"):
        fq.DataModule(tok, train_data_path=tmp_path / "reads.fq.gz", batch_size=12).setup("test")
    with pytest.raises(NotImplementedError, match="no training path"):
        fq.DataModule(tok, train_data_path=golden_dir / "tests.parquet", batch_size=12).setup("fit")
    with pytest.raises(FileNotFoundError):
        fq.DataModule(tok, test_data_path=tmp_path / "absent.parquet", batch_size=12).setup("test")
    with pytest.raises(ValueError, match="test_data_path"):
        fq.DataModule(tok, batch_size=12).setup("test")
    with pytest.raises(NotImplementedError, match="data=fq"):
        bam.BamDataModule(tok, predict_data_path=golden_dir / "test_chimric_reads.bam").setup("test")


def test_fq_yaml_composes_and_instantiates(golden_dir, tmp_path):
    from chimeralm_amd.config import compose, instantiate

    pq_path = str(golden_dir / "tests.parquet")
    cfg = compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt", "data=fq", "model=cnn", "data.batch_size=12",
                                                    f"data.test_data_path={pq_path}"], output_dir=tmp_path)
    assert cfg.data._target_ == "chimeralm_amd.fq.DataModule"
    assert set(cfg.data) >= {"tokenizer", "train_data_path", "val_data_path", "test_data_path", "batch_size",
                             "train_val_test_split", "num_workers", "pin_memory"}
    dm = instantiate(cfg.data)
    assert dm.predict_data_path is None and dm.train_val_test_split == (0.7, 0.2, 0.1)
    dm.setup("test")
    assert sum(b["labels"].shape[0] for b in dm.test_dataloader()) == 25
    # the defaults of eval.yaml stay the BAM predict route
    assert compose(REPO / "configs", "eval.yaml", ["ckpt_path=/x/y.ckpt"], output_dir=tmp_path).data._target_.endswith("BamDataModule")
