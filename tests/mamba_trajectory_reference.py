"""The fp64 reference of the Mamba nets' running verdict (csrc/mamba_verdict.hip, include/chimeralm_hip.h "the running verdict of
the Mamba nets"): the literal definition.  Point k of read b IS the forward of the row cut after its first n_k tokens,

    traj[:, k] = mamba_reference.mamba_forward_fp64(variant, sd, ids[:, :n_k], mask[:, :n_k])

one whole forward per point, so nothing here assumes that the nets are causal: the kernels do, and the comparison tests it.  The
points are `trajectory_reference.points`, the summary is `trajectory_reference.summarize` / `check_summary`."""
from __future__ import annotations

import numpy as np

import mamba_reference as mr
import trajectory_reference as TR


def trajectory_fp64(variant: str, sd: dict, ids: np.ndarray, S: int, mask: np.ndarray | None = None, device=None) -> np.ndarray:
    """[B, K, 2] fp64: the forward of every truncated batch."""
    ids = np.asarray(ids)
    out = [mr.mamba_forward_fp64(variant, sd, ids[:, :n], mask=None if mask is None else np.asarray(mask)[:, :n], device=device)
           .cpu().numpy() for n in TR.points(ids.shape[1], S)]
    return np.stack(out, axis=1)


def sanity_batch(seed: int) -> np.ndarray:
    """Two reads of 777 tokens that end in [SEP], the second behind 300 [PAD]s."""
    ids = mr.synthetic_ids(seed * 100, 2, 777)
    ids[1, :300] = TR.PAD_ID
    ids[:, -1] = TR.SEP_ID
    return ids


def gaps(traj: np.ndarray) -> np.ndarray:
    """[B, K]: logit1 - logit0 at every point."""
    return traj[:, :, 1] - traj[:, :, 0]
