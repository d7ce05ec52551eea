"""Generate tests/golden/eval_golden.json (data only) for the test stage.

Run ONLY in the build container (needs /root/reference and the `datasets` library):   python tests/golden/make_eval_golden.py
The reference's tokenizer module is loaded by file path, as make_golden.py does; nothing of it is copied.  Nothing reaches the
network: the HF libraries are told to stay offline before they are imported.

  parquet   for tests.parquet: number of rows; every row's label by the reference's `parse_target`; the first and last row of
            the test tail that `datasets.load_dataset("parquet", ..., split="train[90%:]")` selects (the library's own percent
            rounding); the `input_ids` shape of the first batch of 12 through the reference's `tokenize_and_align_labels_and_quals`
            and `DataCollator` with `CharacterTokenizer(model_max_length=100, padding_side="left")` (the reference's
            tests/test_data_module.py:55-73 asserts the same shape).
  metrics   three seeded logit / label sets as lists of batches -- "ignored" (rows labelled ignore_index), "one_class" (class 1
            is never predicted) and "uneven" (5 batches of different sizes): per batch torch.nn.CrossEntropyLoss in float64 on
            the fp32 logits, and the confusion counts, by plain torch.  Logits and labels are stored as lists (fp32 values
            print exactly as doubles).
"""
from __future__ import annotations

import os

os.environ["HF_DATASETS_OFFLINE"] = "1"
os.environ["HF_HUB_OFFLINE"] = "1"

import importlib.util  # noqa: E402
import json  # noqa: E402
import tempfile  # noqa: E402
from pathlib import Path  # noqa: E402

import pyarrow.parquet as pq  # noqa: E402
import torch  # noqa: E402

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
IGNORE_INDEX = -100


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, REF / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parquet_golden() -> dict:
    import datasets

    ref = _load("ref_tokenizer", "chimeralm/data/tokenizer.py")
    path = HERE / "tests.parquet"
    rows = pq.read_table(path).to_pylist()
    labels = [ref.parse_target(r["id"])[1] for r in rows]
    with tempfile.TemporaryDirectory() as cache:
        tail = datasets.load_dataset("parquet", data_files={"train": str(path)}, split="train[90%:]", cache_dir=cache)
        tail_ids = list(tail["id"])
    all_ids = [r["id"] for r in rows]
    assert len(set(all_ids)) == len(all_ids)
    first, last = all_ids.index(tail_ids[0]), all_ids.index(tail_ids[-1])
    assert all_ids[first: last + 1] == tail_ids and last == len(rows) - 1
    tok = ref.CharacterTokenizer(model_max_length=100, padding_side="left")
    feats = [ref.tokenize_and_align_labels_and_quals({"id": r["id"], "seq": r["seq"]}, tok, tok.max_len_single_sentence)
             for r in rows[:12]]
    batch = ref.DataCollator(tok).torch_call(feats)
    return {"file": "tests.parquet", "num_rows": len(rows), "labels": labels, "tail_split": "train[90%:]", "tail_first_row": first,
            "tail_last_row": last, "datasets_version": datasets.__version__, "first_batch": {
                "batch_size": 12, "model_max_length": 100, "padding_side": "left", "input_ids_shape": list(batch["input_ids"].shape),
                "labels": batch["labels"].tolist()}}


def _case(name: str, seed: int, sizes: list[int], *, ignore_every: int = 0, never_one: bool = False) -> dict:
    g = torch.Generator().manual_seed(seed)
    batches, tot = [], dict(tp=0, fp=0, tn=0, fn=0, n_valid=0, n_ignored=0)
    loss_fn = torch.nn.CrossEntropyLoss(ignore_index=IGNORE_INDEX)
    sum_loss_fn = torch.nn.CrossEntropyLoss(ignore_index=IGNORE_INDEX, reduction="sum")
    for n in sizes:
        logits = (torch.randn(n, 2, generator=g) * 3.0).float()
        if never_one:
            logits[:, 0] = torch.maximum(logits[:, 0], logits[:, 1] + 0.25)
        labels = torch.randint(0, 2, (n,), generator=g)
        if ignore_every:
            labels[::ignore_every] = IGNORE_INDEX
        valid = labels != IGNORE_INDEX
        pred = torch.argmax(logits, dim=-1)
        c = dict(tp=int(((pred == 1) & (labels == 1) & valid).sum()), fp=int(((pred == 1) & (labels == 0) & valid).sum()),
                 tn=int(((pred == 0) & (labels == 0) & valid).sum()), fn=int(((pred == 0) & (labels == 1) & valid).sum()),
                 n_valid=int(valid.sum()), n_ignored=int((~valid).sum()))
        for k, v in c.items():
            tot[k] += v
        batches.append({"logits": logits.double().tolist(), "labels": labels.tolist(),
                        "mean_loss": float(loss_fn(logits.double(), labels)), "sum_loss": float(sum_loss_fn(logits.double(), labels)),
                        **c})
    return {"name": name, "seed": seed, "ignore_index": IGNORE_INDEX, "batches": batches, "counts": tot,
            "loss": sum(b["mean_loss"] for b in batches) / len(batches),
            "loss_per_read": sum(b["sum_loss"] for b in batches) / tot["n_valid"]}


def main():
    out = {"parquet": parquet_golden(),
           "metrics": [_case("ignored", 11, [12, 12, 7], ignore_every=3), _case("one_class", 12, [16, 9], never_one=True),
                       _case("uneven", 13, [1, 300, 12, 64, 257])]}
    assert out["metrics"][1]["counts"]["tp"] + out["metrics"][1]["counts"]["fp"] == 0
    (HERE / "eval_golden.json").write_text(json.dumps(out, indent=1) + "\n")
    print({k: out["parquet"][k] for k in ("num_rows", "tail_first_row", "tail_last_row")}, out["parquet"]["first_batch"])
    for c in out["metrics"]:
        print(c["name"], c["counts"], c["loss"], c["loss_per_read"])


if __name__ == "__main__":
    main()
