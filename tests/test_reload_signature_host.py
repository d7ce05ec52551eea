"""CPU: when the four modules reload their engine handle.

All four build the reload signature from `(data_ptr, _version)` of every parameter and buffer (chimeralm_amd/_reload.py).  This
pins which edits move it -- and, as a documented limit, the one that does not: an in-place edit through `.data`, which torch's
version counter does not see.  `refresh_weights()` is the way out; the GPU side is tests/test_gpu_handle_history.py."""
from __future__ import annotations

import pytest
import torch
from torch import nn

from chimeralm_amd._reload import reload_signature


def _hyena():
    from chimeralm_amd.hyena import BinarySequenceClassifier, HyenaDna

    net = HyenaDna(2, BinarySequenceClassifier(input_dim=256), precision="fp32")
    return net, net.backbone.backbone.layers[1].mixer.filter_fn.implicit_filter[6].weight, "_engine_sig"


def _transformer():
    from chimeralm_amd.transformer import SequenceCNNTransformer

    net = SequenceCNNTransformer(vocab_size=12, max_len=64, num_encoder_layers=2)
    return net, net.transformer_encoder.layers[1].linear1.weight, "_sig"


def _cnn():
    from chimeralm_amd.cnn import DNAConvNet

    net = DNAConvNet(vocab_size=12, embedding_dim=256, num_filters=[256, 256, 256], kernel_sizes=[7, 7, 7], pool_sizes=[4, 4, 4],
                     hidden_dim=512)
    return net, net.conv_blocks[1][0].weight, "_sig"


def _mamba():
    from chimeralm_amd.mamba import MambaSequenceClassificationSP

    net = MambaSequenceClassificationSP(vocab_size=12, embedding_dim=256, number_of_layers=2, number_of_classes=2, dropout=0.1)
    return net, net.mamba_layers[1].A_log, "_sig"


MODULES = {"hyena": _hyena, "transformer": _transformer, "cnn": _cnn, "mamba": _mamba}


@pytest.mark.parametrize("name", list(MODULES))
def test_reload_signature_follows_counted_edits_and_not_data_edits(name):
    net, p, _ = MODULES[name]()
    sig = reload_signature(net)
    assert sig == reload_signature(net)                          # reading it changes nothing
    assert len(sig) == len(list(net.parameters())) + len(list(net.buffers()))

    def moved(what):
        nonlocal sig
        new = reload_signature(net)
        assert new != sig, f"{name}: the signature did not change after {what}"
        sig = new

    with torch.no_grad():
        p.add_(0.5)
    moved("`with torch.no_grad(): p.add_()`")
    p.detach().mul_(2.0)
    moved("`p.detach().mul_()`")
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    moved("`load_state_dict` of the same values")
    nn.init.normal_(p, std=0.02)
    moved("`nn.init.normal_`")
    p.data = p.data.clone()
    moved("`p.data = t` with a new tensor")
    buffers = list(net.buffers())
    if buffers and buffers[0].is_floating_point():
        with torch.no_grad():
            buffers[0].add_(1.0)
        moved("an in-place edit of a buffer")
    net.to(torch.float64)
    moved("`module.to(dtype)`")
    net.to(torch.float32)
    moved("`module.to(dtype)` back")

    # The documented limit: torch does not count an in-place edit through `.data`, and the storage stays where it is.
    before = p.detach().clone()
    p.data.mul_(3.0)
    p.data[..., 0] = 7.0
    assert not torch.equal(before, p.detach())
    assert reload_signature(net) == sig, f"{name}: `.data` edits are seen now: update INTEGRATION.md and refresh_weights()'s docstring"


@pytest.mark.parametrize("name", list(MODULES))
def test_refresh_weights_drops_the_stored_signature(name):
    """One public method, the same name on all four modules: the next forward finds no stored signature and reloads."""
    net, p, attr = MODULES[name]()
    setattr(net, attr, reload_signature(net))                    # as after a forward
    p.data.mul_(2.0)
    assert getattr(net, attr) == reload_signature(net)           # a forward now would run on the old weights
    assert net.refresh_weights() is None
    assert getattr(net, attr) is None and getattr(net, attr) != reload_signature(net)
