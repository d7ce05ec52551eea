"""Lifecycle of the four engine handles (clm_*, clm_tf_*, clm_cnn_*, clm_mamba_*): create, load, forwards whose second shape
regrows the workspace, close -- three times over.  Every device buffer a handle owns must go with it (free device memory after
cycle 3 within 128 MiB of cycle 1), and a fresh handle on the same weights must compute the same bits."""
import numpy as np
import pytest
import torch

import cnn_reference as cr
import mamba_reference as mr
from oracle import hyena_oracle as ho
from oracle import transformer_oracle as to

pytestmark = pytest.mark.gpu

SLACK = 128 * 2 ** 20


def _free_after(cycle) -> tuple[int, list[torch.Tensor]]:
    out = [t.cpu() for t in cycle()]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0], out


def _three_cycles(cycle):
    free1, ref = _free_after(cycle)
    for _ in range(2):
        free, out = _free_after(cycle)
        assert len(out) == len(ref) and all(torch.equal(a, b) for a, b in zip(out, ref))
    assert abs(free - free1) < SLACK, f"free device memory moved by {(free1 - free) / 2 ** 20:.0f} MiB over two more cycles"


def _hyena_ids(B, L, pads=0):
    ids, _ = ho.synthetic_batch(7, B, L - 1, seed=11)
    ids[:, :pads] = 4
    return torch.from_numpy(ids).cuda()


def test_hyena_engine_lifecycle(built_lib):
    """fp16c; the second batch (128 x 4,097 tokens, 1,500 of them [PAD] on the left) regrows the workspace to ~2 GiB and builds an
    all-[PAD] table; each cycle also runs a self-check and a staged host batch."""
    from chimeralm_amd import _native as N
    from chimeralm_amd.engine import Engine

    sd = ho.make_state_dict(0, head_scale=3.0)
    short, long = _hyena_ids(4, 600), _hyena_ids(128, 4097, pads=1500)
    host = short.cpu().pin_memory()

    def cycle():
        e = Engine("cuda:0", precision="fp16c")
        e.load_state_dict(sd)
        a, b = e.forward(short), e.forward(long)
        diff, differ = e.selfcheck(short)
        k = e.stage_host_ids(host.data_ptr(), N.DT_U8, host.stride(0), *host.shape)
        c = e.forward_staged(k, host.shape[0])
        e.stage_wait(k)
        out = [a, b, c, torch.tensor([diff, differ])]
        torch.cuda.synchronize()
        e.close()
        return out

    _three_cycles(cycle)


def test_transformer_lifecycle(built_lib):
    from chimeralm_amd.transformer import SequenceCNNTransformer

    sd = to.make_state_dict(5, to.PRODUCTION, scale=1.0)
    short = torch.from_numpy(to.synthetic_ids(1, 4, 1000, 40)).cuda()
    long = torch.from_numpy(to.synthetic_ids(2, 8, 4101, 7)).cuda()

    def cycle():
        net = SequenceCNNTransformer(vocab_size=12, max_len=32768, num_encoder_layers=12, precision="fp16x3", selfcheck=False)
        net.load_state_dict(sd, strict=True)
        out = [net(short), net(long)]
        torch.cuda.synchronize()
        net.close()
        return out

    _three_cycles(cycle)


def test_cnn_lifecycle(built_lib):
    from chimeralm_amd.cnn import DNAConvNet

    sd = cr.make_cnn_state_dict(5)
    short = torch.from_numpy(cr.synthetic_ids(1, 2, 777, 30)).cuda()
    long = torch.from_numpy(cr.synthetic_ids(2, 4, 8193, 100)).cuda()

    def cycle():
        net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                         hidden_dim=512, number_of_classes=2, dropout=0.1, precision="fp16x3")
        net.load_state_dict(sd, strict=True)
        out = [net(short), net(long)]
        torch.cuda.synchronize()
        net.close()
        return out

    _three_cycles(cycle)


def test_mamba_lifecycle(built_lib):
    from chimeralm_amd.mamba import MambaSequenceClassificationSP

    sd = mr.make_mamba_state_dict("mambasp", 5, n_layers=2, d_model=256)
    short = torch.from_numpy(mr.synthetic_ids(1, 2, 300, 30)).cuda()
    long = torch.from_numpy(mr.synthetic_ids(2, 4, 2100, 100)).cuda()

    def cycle():
        net = MambaSequenceClassificationSP(vocab_size=12, embedding_dim=256, number_of_layers=2, number_of_classes=2, dropout=0.2,
                                            d_state=mr.VARIANTS["mambasp"][2], expand=mr.VARIANTS["mambasp"][3], precision="fp16x3")
        net.load_state_dict(sd, strict=True)
        out = [net(short), net(long)]
        torch.cuda.synchronize()
        net.close()
        return out

    _three_cycles(cycle)
