"""Long-read tiling restated in numpy from the definitions in include/chimeralm_hip.h: the windows of a read by brute force, the
plan, the rows a plan stands for, the head batch, and the reduction.  Shared by test_longread_host.py and test_gpu_longread.py."""
import numpy as np

PAD, SEP = 4, 1


def window_starts(n, wb, overlap):
    """First bases of the windows of a read of n bases (after the cap), by walking: a window every `step` bases while it does not
    reach the read's end, and one right-aligned on the last base."""
    if n <= wb:
        return [0]
    step = wb - overlap
    starts, at = [], 0
    while at + wb < n:
        starts.append(at)
        at += step
    return starts + [n - wb]


def np_plan(lengths, L, wb, overlap, max_bases):
    """(L_out, first [B + 1], spans [(read, src_col, n_copy, sep)], starts) for rows of `lengths` tokens of L: the B head rows first,
    then the extra windows in read order, then window order."""
    B = len(lengths)
    head, extra, head_starts, extra_starts, first = [], [], [], [], [0]
    for r, nt in enumerate(int(x) for x in lengths):
        nb, col0 = nt - 1, L - nt
        if nb <= wb:
            head.append((r, col0, nt, 0))
            head_starts.append(0)
            first.append(first[-1])
            continue
        st = window_starts(min(nb, max_bases), wb, overlap)
        head.append((r, col0, wb, 1))
        head_starts.append(0)
        extra += [(r, col0 + s, wb, 1) for s in st[1:]]
        extra_starts += st[1:]
        first.append(first[-1] + len(st) - 1)
    assert len(head) == B
    return min(L, wb + 1), np.asarray(first, np.int32), head + extra, np.asarray(head_starts + extra_starts, np.int32)


def np_rows(ids, spans, width):
    """The rows the spans stand for: [PAD] x (width - n_copy - sep), the copied bytes, [SEP] if sep."""
    out = np.full((len(spans), width), PAD, dtype=np.uint8)
    for i, (r, col, n, sep) in enumerate(spans):
        out[i, width - n - sep: width - sep] = ids[r, col: col + n]
        if sep:
            out[i, width - 1] = SEP
    return out


def np_lengths(ids):
    return (ids != PAD).sum(1).astype(np.int32)


def np_head_batch(ids, wb, overlap=0, max_bases=None):
    """The head batch of an untruncated left-padded batch: what the truncating path delivers."""
    L = ids.shape[1]
    L_out, _first, spans, _starts = np_plan(np_lengths(ids), L, wb, overlap, max_bases if max_bases is not None else max(L, wb))
    return np_rows(ids, spans[: ids.shape[0]], L_out)


def np_reduce(logits, first, B):
    """(logits_out [B, 2] as the chosen rows, chosen [B], gap [B + n_extra] fp32, nonfinite [B]) from fp32 logits [B + n_extra, 2]:
    the largest float64 gap, equal gaps to the lowest window; the lowest window with a non-finite logit if there is one."""
    logits = np.asarray(logits, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        gap64 = logits[:, 1].astype(np.float64) - logits[:, 0].astype(np.float64)
    fin = np.isfinite(logits).all(1)
    out = np.zeros((B, 2), dtype=np.float32)
    chosen, bad = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for r in range(B):
        rows = [r] + list(range(B + int(first[r]), B + int(first[r + 1])))
        nf = [k for k, i in enumerate(rows) if not fin[i]]
        bad[r] = len(nf)
        if nf:
            k = nf[0]
        else:
            k = 0
            for j in range(1, len(rows)):
                if gap64[rows[j]] > gap64[rows[k]]:
                    k = j
        chosen[r] = k
        out[r] = logits[rows[k]]
    with np.errstate(over="ignore"):
        return out, chosen, gap64.astype(np.float32), bad


def make_batch(n_bases, seed, L=None):
    """A left-padded uint8 batch of seeded reads of `n_bases` bases each (A, C, G, T), every one followed by [SEP]."""
    rng = np.random.default_rng(seed)
    L = L if L is not None else max(n_bases) + 1
    ids = np.full((len(n_bases), L), PAD, dtype=np.uint8)
    for r, n in enumerate(n_bases):
        ids[r, L - n - 1: L - 1] = 7 + rng.integers(0, 4, size=n)
        ids[r, L - 1] = SEP
    return ids
