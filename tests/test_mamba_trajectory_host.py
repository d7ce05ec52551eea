"""CPU: the Mamba nets' running verdict -- ABI, kernel resources, module knobs, loop and eval.py refusals, and that the fp64 reference
moves (csrc/mamba_verdict.hip; the GPU side: test_gpu_mamba_trajectory.py)."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mamba_trajectory_reference as MT
import mamba_reference as mr
import trajectory_reference as TR

REPO = Path(__file__).resolve().parent.parent


def _net(variant, **kw):
    from chimeralm_amd import mamba

    if variant == "mamba":
        return mamba.MambaSequenceClassification(vocab_size=12, embedding_dim=256, number_of_layers=1, model_max_length=512, dropout=0.1,
                                                 number_of_classes=2, d_state=16, **kw)
    return mamba.MambaSequenceClassificationSP(vocab_size=12, embedding_dim=256, number_of_layers=1, number_of_classes=2, dropout=0.1,
                                               d_state=16, **kw)


# ------------------------------------------------------------------------------------------------ ABI and kernels
def test_header_native_and_exports(built_lib):
    from chimeralm_amd import _native as N, build

    header = (REPO / "include" / "chimeralm_hip.h").read_text()
    lib = ctypes.CDLL(str(built_lib))
    name = "clm_mamba_forward_traj"
    assert hasattr(lib, name) and name in N.SYMBOLS and f"int {name}(" in header
    assert len(N.SYMBOLS[name][1]) == len(N.SYMBOLS["clm_mamba_forward"][1]) + 1
    assert N.SYMBOLS[name][1][-2] == ctypes.POINTER(N.ClmTrajOut)
    assert "#define CLM_ABI_VERSION 6" in header and N.ABI_VERSION == 6 and lib.clm_abi_version() == 6   # a new symbol only
    assert "mamba_verdict.hip" in build.SOURCES
    for text in ("The mean divides by n_k, pads and masked rows included", "copied bit for bit", "does not end in [SEP]",
                 "describe pads only", "fp32 or fp16x3"):
        assert text in header, text


def test_new_kernels_have_no_scratch_and_stay_out_of_the_counted_patterns(built_lib):
    from chimeralm_amd import build

    blocks = {b.splitlines()[0].strip(): b for b in build.RESOURCES.read_text().split("Function Name: ")[1:]}
    new = {n: b for n, b in blocks.items() if "ssm_verdict_" in n}
    assert sum("ssm_verdict_pool_kernel" in n for n in new) == 1
    assert sum("ssm_verdict_head_kernel" in n for n in new) == 2                # d_model 256 and 512
    assert len(new) == 3
    for n, b in new.items():
        assert re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1) == "0", n
        assert not re.search(r"mamba_[a-z_]+_kernel", n), n                     # test_mamba_host.py counts these: 18
        assert "traj_" not in n, n                                              # test_trajectory_host.py counts these: 3
    assert sum(bool(re.search(r"mamba_[a-z_]+_kernel", n)) for n in blocks) == 18
    assert sum("traj_" in n for n in blocks) == 3


# ------------------------------------------------------------------------------------------------ the modules
@pytest.mark.parametrize("variant", ["mamba", "mambasp"])
def test_module_knobs(variant):
    from chimeralm_amd.engine import TrajectoryRequest

    plain = _net(variant)
    assert plain.trajectory_stride is None and plain.trajectory_request() is None and plain.last_trajectory is None
    net = _net(variant, trajectory_stride=256)
    assert net.trajectory_stride == 256 and net.trajectory_request() == TrajectoryRequest(256, True) and net.last_trajectory is None
    assert _net(variant, trajectory_stride=4096).trajectory_request().stride == 4096
    for bad in (0, 64, 192, 8192):
        with pytest.raises(ValueError, match="multiple of 128"):
            _net(variant, trajectory_stride=bad)
    import inspect

    assert inspect.signature(type(net).__init__).parameters["trajectory_stride"].kind is inspect.Parameter.KEYWORD_ONLY
    assert set(net.state_dict()) == set(plain.state_dict())                     # a knob, not a parameter


# ------------------------------------------------------------------------------------------------ the loops
def test_loops_take_the_mamba_nets_and_keep_their_refusals(tmp_path):
    from chimeralm_amd import cnn, lm, longread, predict
    from chimeralm_amd.callbacks import PredictionWriter, TrajectoryWriter

    tw, dev = TrajectoryWriter(tmp_path), torch.device("cpu")
    for variant, stride in (("mamba", 128), ("mambasp", 384)):
        model = SimpleNamespace(net=_net(variant, trajectory_stride=stride))
        req = predict._trajectory_setup(model, tw)
        assert req.stride == stride and req.summary
        assert predict._trajectory_setup(model, None) is None
        with pytest.raises(ValueError, match="trajectory_stride"):
            predict._trajectory_setup(SimpleNamespace(net=_net(variant)), tw)
        tile = longread.Options(mode="tile", window=1024, overlap=128, max_bases=4096)
        with pytest.raises(ValueError, match="single row"):
            predict._trajectory_setup(model, tw, tile)
        with pytest.raises(ValueError, match="single row"):
            predict.run_predict(model, None, PredictionWriter(tmp_path), dev, trajectory_writer=tw, long_reads=tile)
    conv = SimpleNamespace(net=cnn.DNAConvNet(**cnn.PRODUCTION))
    with pytest.raises(ValueError, match="causal") as e:
        predict._trajectory_setup(conv, tw)
    assert "not built" not in str(e.value) and "Mamba" in str(e.value)
    with pytest.raises(ValueError, match="causal"):
        predict.run_predict(conv, None, PredictionWriter(tmp_path), dev, trajectory_writer=tw)
    assert predict._trajectory_setup(lm.ChimeraLM.new(trajectory_stride=128), tw).stride == 128      # Hyena as before


# ------------------------------------------------------------------------------------------------ eval.py
def test_eval_py_trajectory_keys():
    import eval as ev

    assert ev.trajectory_options({}) is None and ev.trajectory_options({"trajectory": {}}) is None
    assert ev.trajectory_options({"trajectory": {"stride": 128}}) == (128, False)
    assert ev.trajectory_options({"trajectory": {"stride": 4096, "values": True}}) == (4096, True)
    with pytest.raises(ValueError, match="step"):
        ev.trajectory_options({"trajectory": {"stride": 128, "step": 3}})
    for bad in (0, 64, 192, 8192):
        with pytest.raises(ValueError, match="multiple of 128"):
            ev.trajectory_options({"trajectory": {"stride": bad}})
    for bad in ({"values": True}, {"stride": "wide"}, {"stride": True}, {"stride": 128.0}):
        with pytest.raises(ValueError, match="stride"):
            ev.trajectory_options({"trajectory": bad})
    with pytest.raises(ValueError, match="values"):
        ev.trajectory_options({"trajectory": {"stride": 128, "values": "all"}})


def test_eval_py_refuses_tiling_and_the_test_route(tmp_path):
    import eval as ev

    common = [f"ckpt_path={tmp_path / 'none.ckpt'}", "model=mambasp", f"hydra.run.dir={tmp_path / 'run'}", "+trajectory.stride=128"]
    with pytest.raises(ValueError, match="exclude each other"):
        ev.main(common + [f"+data.predict_data_path={tmp_path / 'none.bam'}", "+long_reads.mode=tile"])
    with pytest.raises(ValueError, match=r"\+trajectory.stride belongs to the predict route"):
        ev.main(common + ["data=fq", f"data.test_data_path={tmp_path / 'none.parquet'}"])
    with pytest.raises(ValueError, match="unknown trajectory option"):
        ev.main(common + [f"+data.predict_data_path={tmp_path / 'none.bam'}", "+trajectory.every=2"])
    with pytest.raises(ValueError, match="multiple of 128"):
        ev.main([a for a in common if "trajectory" not in a] + [f"+data.predict_data_path={tmp_path / 'none.bam'}", "+trajectory.stride=192"])


def test_trainer_predict_takes_a_trajectory_writer():
    import inspect

    from chimeralm_amd.trainer import Trainer

    p = inspect.signature(Trainer.predict).parameters["trajectory_writer"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


# ------------------------------------------------------------------------------------------------ the reference says something
@pytest.mark.parametrize("variant,seed", [("mamba", 31), ("mambasp", 32)])
def test_reference_curve_moves(variant, seed):
    """The literal fp64 trajectory at S = 128 of two reads of 777 tokens (one behind 300 pads): the gap moves between neighbouring
    points, and row 1 of `mambasp` changes its label along the way -- so the GPU comparison per point says something."""
    sd = mr.make_mamba_state_dict(variant, seed)
    ids = MT.sanity_batch(seed)
    ref = MT.trajectory_fp64(variant, sd, ids, 128)
    assert ref.shape == (2, 7, 2) and TR.points(777, 128)[-1] == 777
    assert np.abs(ref[:, -1] - mr.mamba_forward_fp64(variant, sd, ids).numpy()).max() == 0.0
    g = MT.gaps(ref)
    steps = np.abs(np.diff(g, axis=1))
    print(f"{variant}: |gap step| between neighbouring points from {steps.min():.2e} to {steps.max():.2e}; labels {(g > 0).astype(int).tolist()}")
    assert steps.max() > 1e-3
    if variant == "mambasp":
        labels = g[1] > 0
        assert labels.any() and not labels.all()                                # a label flip along row 1
