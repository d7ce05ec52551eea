"""When a module reloads its engine handle: the signature all four nets compare between forwards.

`(data_ptr, _version)` of every parameter and buffer.  It changes when a tensor is replaced (`load_state_dict` into new storage,
`p.data = t`, `module.to(dtype)`) and when autograd's version counter moves (`with torch.no_grad(): p.add_()`,
`p.detach().add_()`, `load_state_dict`, `nn.init.*`).  It does NOT change for an in-place edit through `.data`
(`p.data.mul_(2)`): torch does not count those, and finding them would take a content hash or a device sync per forward.
After such an edit call the module's `refresh_weights()`.
"""
from __future__ import annotations

from torch import nn


def reload_signature(module: nn.Module) -> tuple:
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))
