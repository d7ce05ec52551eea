"""Train the two Mamba nets on one MI355X (the reference's `train.py` with `model=mamba` / `model=mambasp`; the reference's
chimeralm/models/components/mamba.py in `train()`, basic_module.py `training_step`).

`mamba_ssm.Mamba2` is CUDA / Triton only.  Here the core of the layer -- the causal depthwise conv + SiLU, the dt softplus, the
chunked state-space scan with the D skip, the gate and the gated RMSNorm -- runs forward and backward in the engine
(csrc/mamba_train.hip, `clm_mamba_train_*`), wrapped as `Mamba2Core`, a `torch.autograd.Function` on the module's CURRENT parameters.
Everything around it is ordinary differentiable torch on the module's own tensors: the embedding (torch's `padding_idx` rule),
`mamba`'s positional term, Linear, LayerNorm and masks, in_proj and out_proj (`F.linear`, i.e. rocBLAS), the residuals, dropout,
(mean + max) / 2 pooling, pooler and classifier.

The op is stateless across calls: what a backward needs (zxbcdt, the conv output, dt, the scan output and every chunk's entry state)
are torch tensors held by the autograd node, so a net of 3 or 12 layers has 3 or 12 live nodes and no rule about their order.

Deliberate differences from the reference: dropout masks come from torch's generator, not the reference's stream;
the training arithmetic is exact fp32 whatever the module's inference `precision`; `Mamba2`'s internals are restated, not pinned.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _native as N
from ._trainop import is_plain_fp32, stream_of
from .mamba import HEADDIM, VOCAB

N_PARAMS = 6                                 # conv1d.weight, conv1d.bias, dt_bias, A_log, D, norm.weight: CLM_MAMBA_TRAIN_PARAMS
Q = 64                                       # tokens per scan chunk: one entry state each (csrc/mamba_common.h)


class MambaTrainError(RuntimeError):
    pass


def core_parameters(layer) -> list[torch.nn.Parameter]:
    """The parameters of a `mamba.Mamba2` the engine differentiates, in the ABI's order."""
    return [layer.conv1d.weight, layer.conv1d.bias, layer.dt_bias, layer.A_log, layer.D, layer.norm.weight]


def workspace_bytes(B: int, L: int, d_model: int, expand: int, d_state: int) -> int:
    """Bytes of engine scratch one backward of that shape takes (the formula of include/chimeralm_hip.h)."""
    return int(N.load().clm_mamba_train_workspace_bytes(B, L, d_model, expand, d_state))


class MambaTrainEngine:
    """One `clm_mamba_train_handle`: the device, the error string and the backward's scratch."""

    def __init__(self, device: torch.device):
        self.lib = N.load()
        self.device = device
        h = C.c_void_p()
        dev = device.index if device.index is not None else torch.cuda.current_device()
        if self.lib.clm_mamba_train_create(dev, C.byref(h)) != 0:
            raise MambaTrainError(self.lib.clm_mamba_train_last_error(None).decode())
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            raise MambaTrainError(self.lib.clm_mamba_train_last_error(self._h).decode())

    @staticmethod
    def _ptrs(ts):
        return (C.c_void_p * N_PARAMS)(*[t.data_ptr() for t in ts])

    @staticmethod
    def _checked(zx, params):
        if not all(is_plain_fp32(t, zx.device) for t in [zx, *params]):
            raise ValueError("the engine trains contiguous fp32 tensors on one device")

    def forward(self, zx: torch.Tensor, params: list[torch.Tensor], d_model: int, expand: int, d_state: int):
        """-> out [B, L, di] and what the backward needs: (xc [B, L, di + 2 N], dt [B, L, H], ys [B, L, di], states [B, H, chunks, N, 64])."""
        self._checked(zx, params)
        B, L, _ = zx.shape
        di = expand * d_model
        H = di // HEADDIM
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=zx.device)   # noqa: E731
        xc, dt, ys, out = new(B, L, di + 2 * d_state), new(B, L, H), new(B, L, di), new(B, L, di)
        states = new(B, H, (L + Q - 1) // Q, d_state, HEADDIM)
        self._check(self.lib.clm_mamba_train_forward(self._h, zx.data_ptr(), self._ptrs(params), B, L, d_model, expand, d_state, xc.data_ptr(),
                                                     dt.data_ptr(), ys.data_ptr(), states.data_ptr(), out.data_ptr(), stream_of(self.device)))
        return out, (xc, dt, ys, states)

    def backward(self, zx, params, saved, dout, d_model: int, expand: int, d_state: int):
        """-> dzxbcdt and the six parameter gradients."""
        self._checked(zx, params)
        B, L, _ = zx.shape
        xc, dt, ys, states = saved
        dzx = torch.empty_like(zx)
        grads = [torch.empty_like(p) for p in params]
        self._check(self.lib.clm_mamba_train_backward(self._h, zx.data_ptr(), self._ptrs(params), B, L, d_model, expand, d_state, xc.data_ptr(),
                                                      dt.data_ptr(), ys.data_ptr(), states.data_ptr(), dout.data_ptr(), dzx.data_ptr(),
                                                      self._ptrs(grads), stream_of(self.device)))
        return dzx, grads

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.clm_mamba_train_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mamba2Core(torch.autograd.Function):
    """out [B, L, d_inner] of zxbcdt [B, L, 2 d_inner + 2 N + H] (the raw in_proj output) under the six core parameters, differentiable
    in all seven.  `dims` = (d_model, expand, d_state)."""

    @staticmethod
    def forward(ctx, eng, dims, zxbcdt, *params):
        zx = zxbcdt.detach().contiguous()
        det = [p.detach() for p in params]
        out, saved = eng.forward(zx, det, *dims)
        ctx.eng, ctx.dims, ctx.zx, ctx.det, ctx.saved = eng, dims, zx, det, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        dzx, grads = ctx.eng.backward(ctx.zx, ctx.det, ctx.saved, dout.contiguous().float(), *ctx.dims)
        return (None, None, dzx, *grads)


def mamba2_layer(eng, layer, h: torch.Tensor) -> torch.Tensor:
    """`mamba_ssm.Mamba2.forward` of `layer` (a `mamba.Mamba2`) on h [B, L, d_model]: in_proj and out_proj in torch, the core on the engine."""
    zx = F.linear(h, layer.in_proj.weight)
    y = Mamba2Core.apply(eng, (layer.d_model, layer.expand, layer.d_state), zx, *core_parameters(layer))
    return F.linear(y, layer.out_proj.weight)


def train_forward(net, input_ids: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
    """logits [B, 2] of `net` (a Mamba net with `trainable=True`, in training mode) with a graph to every parameter.  The pooled
    vector and the positions the max-pool took are left in `net.last_train_pooled` / `net.last_train_route` (detached)."""
    dev = input_ids.device
    eng = net.train_engine(dev)
    ids = input_ids.long().clamp(0, VOCAB - 1)                       # (the inference kernels clamp too)
    h = net.embedding(ids)
    m = None
    if hasattr(net, "input_block"):                                  # `mamba`: positional term, Linear + LayerNorm + Dropout, mask
        h = net.input_block(h + net.pos_embedding[:, :ids.shape[1]])
        if mask is not None:
            m = mask.to(device=dev, dtype=h.dtype).unsqueeze(-1)
            h = h * m
    for entry in net.mamba_layers:
        if isinstance(entry, torch.nn.ModuleDict):
            h = h + entry["dropout"](mamba2_layer(eng, entry["mamba"], h))
        else:
            h = h + mamba2_layer(eng, entry, h)
        if m is not None:
            h = h * m
    mx, route = h.max(dim=1)
    pooled = (h.mean(dim=1) + mx) / 2
    net.last_train_pooled, net.last_train_route = pooled.detach(), route
    return net.classifier(net.pooler(pooled))


# ------------------------------------------------------------------------------------------------------------- the loop
def fit_mamba(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 8, lr: float | None = None, seed: int = 12345,
              device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train every parameter of `model.net` (a `ClassificationLit` over a Mamba net with `trainable=True`) on one GPU: `fit.fit` with
    `fit.whole_batch_step` -- nothing here couples the reads of a batch, so a batch of one read trains.  Optimizer and scheduler are
    the model's factories (configs/model/mamba.yaml, mambasp.yaml); dropout draws from torch's generator, seeded here with `seed`."""
    from . import fit

    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be >= 1")
    torch.manual_seed(int(seed))                                     # the dropout masks
    return fit.fit(model, train_rows, val_rows, out_dir, params=fit.trainable_parameters(model.net, "net"), step=fit.whole_batch_step,
                   min_reads=1, config="configs/model/mamba.yaml, mambasp.yaml", epochs=epochs, batch_size=batch_size, lr=lr, seed=seed,
                   device=device, tokenizer=tokenizer, metrics_factory=metrics_factory)
