"""References for the running verdict (csrc/trajectory.hip, include/chimeralm_hip.h "the running verdict"):

`trajectory_fp64`  the oracle's head on the first n_k rows of the oracle's final residual stream, in fp64, per point;
`summarize`        the per-read summary as a function of a trajectory [K, 2] and the row's ids, in numpy -- what the kernel's
                   one-thread-per-read loop computes, written the long way round (forwards, from the definitions)."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import hyena_oracle as ho

PAD_ID, SEP_ID = 4, 1
FIELDS = ("n_pad", "n_bases", "has_sep", "n_points", "first_k", "label", "onset_k", "jump_k", "n_nonfinite", "reserved",
          "jump_dgap", "final_gap")


def points(L: int, S: int) -> list[int]:
    """n_k of the K = ceil(L / S) points of a row of L tokens."""
    K = -(-L // S)
    return [min((k + 1) * S, L) for k in range(K)]


def trajectory_fp64(ids: np.ndarray, sd: dict, S: int) -> np.ndarray:
    """[B, K, 2] fp64: head_forward(backbone_forward(ids)[:, :n_k]) per point."""
    t = torch.from_numpy(np.asarray(ids).astype(np.int64))
    with torch.no_grad():
        hidden = ho.backbone_forward(t, sd, torch.float64)
        return torch.stack([ho.head_forward(hidden[:, :n], sd, torch.float64) for n in points(t.shape[1], S)], dim=1).numpy()


def padded_batch(L: int, prefixes, seed: int) -> np.ndarray:
    """Seeded reads of L tokens that end in [SEP], read b left-padded with prefixes[b] [PAD]s."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(7, 11, size=(len(prefixes), L)).astype(np.uint8)
    ids[:, -1] = SEP_ID
    for b, p in enumerate(prefixes):
        ids[b, :p] = PAD_ID
    return ids


# the shapes of the GPU tests: name -> (ids, S, chunk_reads)
def case(name: str):
    if name == "3x1":
        return np.array([[1], [4], [8]], np.uint8), 128, 256        # [SEP] alone, [PAD] alone, one base without [SEP]: K = 1
    B, L, S, chunk, prefixes = {
        "2x128": (2, 128, 128, 256, (0, 5)),
        "2x129": (2, 129, 128, 256, (0, 128)),                       # the peeled slot (16-bit path); one read: [SEP] alone behind pads
        "2x130": (2, 130, 128, 256, (0, 127)),
        "3x257": (3, 257, 128, 256, (0, 129, 256)),
        "5x300": (5, 300, 128, 256, (260, 0, 3, 130, 129)),          # a read of 40 tokens: two whole [PAD] tiles from the table
        "5x300s256": (5, 300, 256, 256, (260, 0, 3, 130, 129)),
        "6x300c4": (6, 300, 128, 4, (0, 260, 128, 1, 299, 140)),     # two chunks: row offsets; 4 x 2 and 2 x 2 interior rows, the last not a multiple of 8
        "2x8193": (2, 8193, 128, 256, (0, 5000)),
    }[name]
    return padded_batch(L, prefixes, seed=1000 + L + B), S, chunk


@functools.lru_cache(maxsize=None)
def case_reference(name: str, head_scale: float = 3.0) -> np.ndarray:
    """The fp64 trajectory of a case under make_state_dict(0, head_scale): computed once, shared by the tests, never written to."""
    ids, S, _ = case(name)
    ref = trajectory_fp64(ids, ho.make_state_dict(0, head_scale=head_scale), S)
    ref.setflags(write=False)
    return ref


def bases_seen(K: int, S: int, L: int, n_pad: int, n_bases: int) -> list[int]:
    return [int(min(max(min((k + 1) * S, L) - n_pad, 0), n_bases)) for k in range(K)]


def summarize(traj: np.ndarray, ids_row: np.ndarray, S: int) -> dict:
    """The summary record of one read from its trajectory fp32 [K, 2] and its ids [L]."""
    traj = np.asarray(traj, np.float32)
    L, K = len(ids_row), traj.shape[0]
    assert K == -(-L // S)
    not_pad = np.flatnonzero(np.asarray(ids_row) != PAD_ID)
    n_pad = int(not_pad[0]) if len(not_pad) else L
    has_sep = int(ids_row[-1] == SEP_ID)
    n_bases = max(0, L - n_pad - has_sep)
    n_k = points(L, S)
    first_k = next((k for k in range(K) if n_k[k] > n_pad), K - 1)
    gap = traj[:, 1].astype(np.float64) - traj[:, 0].astype(np.float64)
    label = int(gap[K - 1] > 0)
    has = [int(g > 0) == label for g in gap]
    informative = range(first_k, K)
    n_nonfinite = sum(1 for k in informative if not np.isfinite(traj[k]).all())
    onset_k = min(k for k in informative if all(has[k:]))
    sgn = 1.0 if label else -1.0
    jump_k, jump_dgap = -1, 0.0
    for k in range(first_k + 1, K):
        d = sgn * (gap[k] - gap[k - 1])
        if jump_k < 0 or d > jump_dgap:                              # strictly larger: ties go to the lowest k
            jump_k, jump_dgap = k, d
    if n_nonfinite:
        onset_k, jump_k, jump_dgap = -1, -1, 0.0
    return dict(n_pad=n_pad, n_bases=n_bases, has_sep=has_sep, n_points=K, first_k=first_k, label=label, onset_k=onset_k, jump_k=jump_k,
                n_nonfinite=n_nonfinite, reserved=0, jump_dgap=np.float32(jump_dgap), final_gap=np.float32(gap[K - 1]))


def check_summary(summary_i32: np.ndarray, traj: np.ndarray, ids: np.ndarray, S: int) -> None:
    """The device's records int32 [B, 12] (two fp32 columns viewed as int32) against `summarize` of the device's own trajectory:
    a discrete function, so every field of every read, bit for bit."""
    f32 = summary_i32.view(np.float32)
    for b in range(len(ids)):
        want = summarize(traj[b], ids[b], S)
        got = {n: (np.float32(f32[b, i]) if i >= 10 else int(summary_i32[b, i])) for i, n in enumerate(FIELDS)}
        for n in FIELDS:
            same = got[n] == want[n] or (i_nan(got[n]) and i_nan(want[n]))
            assert same, (b, n, got, want)


def i_nan(v) -> bool:
    return isinstance(v, (float, np.floating)) and bool(np.isnan(v))
