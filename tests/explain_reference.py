"""The mutagenesis scan restated in numpy from the definition in include/chimeralm_hip.h: seeded reads, the brute-force mutant
enumeration, the rows a plan stands for, and the scores and reduce kernels.  Shared by test_explain_host.py and test_gpu_explain.py."""
import numpy as np


def make_read(n_bases, seed, with_n=False):
    rng = np.random.default_rng(seed)
    ids = (7 + rng.integers(0, 4, size=n_bases)).astype(np.uint8)
    if with_n:
        ids[rng.integers(0, n_bases, size=max(1, n_bases // 16))] = 11
    return np.concatenate([ids, np.array([1], np.uint8)])


def brute_force_plan(ids, w, s, substitute):
    """(start, sub, slot) per mutant and n_windows, from the definition: window k starts at base k * s, n_windows = ceil(n / s);
    "N": one mutant per window, slot k; "all": per base the columns A, C, G, T except the base's own, slot 4 k + column."""
    n = len(ids) - 1
    n_windows = -(-n // s)
    out = []
    for k in range(n_windows):
        if substitute == "N":
            out.append((k * s, 11, k))
        else:
            out += [(k, 7 + c, 4 * k + c) for c in range(4) if ids[k] != 7 + c]
    return out, n_windows


def mutant_rows(ids, plan, w):
    """The rows the plan stands for, built on the host: bases [start, min(start + w, n_bases)) replaced, [SEP] kept."""
    n = len(ids) - 1
    rows = np.tile(ids, (len(plan), 1))
    for m, (start, sub, _slot) in enumerate(plan):
        rows[m, start:min(start + w, n)] = sub
    return rows


def np_scores(logits):
    """dp1, dgap per mutant in float64 from logits [M + 1, 2] (row 0 the read): the header's definition."""
    l = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore"):                       # (a crafted inf logit: its row is NaN, as the kernel's)
        m = l.max(1, keepdims=True)
        e = np.exp(l - m)
        p1 = e[:, 1] / e.sum(1)
        gap = l[:, 1] - l[:, 0]
        return p1[1:] - p1[0], gap[1:] - gap[0]


def np_reduce(d, n_bases, w, s, top_k):
    """importance [n_bases] and the peaks from d [n_windows, S]: maximum of |d| over covering windows and columns, NaN if any is
    NaN; peaks by descending value, equal values by position; none if anything is NaN."""
    a = np.abs(np.asarray(d, dtype=np.float32))
    win = np.where(np.isnan(a).any(1), np.float32(np.nan), a.max(1))
    imp = np.full(n_bases, -1.0, dtype=np.float32)
    for k in range(len(win)):
        seg = slice(k * s, min(k * s + w, n_bases))
        imp[seg] = np.where(np.isnan(imp[seg]) | np.isnan(win[k]), np.float32(np.nan), np.maximum(imp[seg], win[k]))
    pos, val = np.full(top_k, -1, dtype=np.int32), np.zeros(top_k, dtype=np.float32)
    if not np.isnan(imp).any():
        order = np.lexsort((np.arange(n_bases), -imp))[: min(top_k, n_bases)]
        pos[: len(order)], val[: len(order)] = order, imp[order]
    return imp, pos, val


def host_batches(ids, plan, w, batch_size):
    """The batches the scan runs, built on the host: the read first, then the mutants in plan order."""
    rows = np.concatenate([ids[None, :], mutant_rows(ids, plan, w)])
    return [rows[i:i + batch_size] for i in range(0, len(rows), batch_size)]


