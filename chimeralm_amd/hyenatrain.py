"""Fine-tune the whole HyenaDna net on one MI355X (the reference's `train.py model=hyena` with `freeze_backbone=False`, its default;
/root/reference/chimeralm/models/components/hyena.py:218-256, basic_module.py `training_step`).

The core of the Hyena operator -- the causal 3-tap filter, the two gates and the FFT long convolution with its skip term -- runs
forward and backward in the engine (csrc/hyena_train.hip, `clm_hyena_train_*`), wrapped as `HyenaCore`, a `torch.autograd.Function`
differentiable in the raw in_proj output, the short filter's parameters, the modulated implicit filter k and the skip D.  Everything
around it is ordinary differentiable torch on the module's own parameter containers: the embedding and its dropout, the LayerNorms,
in_proj / out_proj (computed channel-major, so that no transposing copy stands between them and the core), the GELU-tanh MLP, the
implicit-filter MLP with its sines (autograd carries dk on into it, `freq` and `pos_emb.z`) and the head.

The op is stateless: four layers make four live autograd nodes that keep zc, c and the parameters as torch tensors.

`hyena_core="torch"` swaps the op for `F.conv1d` and `rfft` / `irfft` at n = 2 L, as the reference's `fftconv` does: the comparison
path, the path of reads beyond the op's 8,193 tokens (taken automatically, logged once, visible in `net.last_train_core`) and a
forward that runs on CPU tensors.

`hyena_long_core="engine"` (default "torch") sends reads of 8,194 ... 32,769 tokens to the segmented op instead
(csrc/hyena_longtrain.hip, `clm_hyena_longtrain_*`, `HyenaLongCore`; `net.last_train_core == "engine-long"`): the same operator over
8,192-token segments.

Deliberate differences from the reference: the embedding dropout is drawn from `net.dropout_generator`, not the
reference's stream; the training arithmetic is exact fp32 whatever the module's inference `precision`; the backbone is the restated
HyenaDNA algorithm, not the Hub's remote code, which the reference does not pin either.
"""
from __future__ import annotations

import logging

import torch
import torch.nn.functional as F

from . import _native as N
from ._trainop import abi_error, inverted_dropout, is_plain_fp32, stream_of
from .headtrain import head_mlp

log = logging.getLogger("chimeralm_amd")
DM = 256
MAX_ENGINE_TOKENS = 8193                     # one power-of-two transform of at most 16384 points (include/chimeralm_hip.h)
MAX_LONG_TOKENS = 32769                      # the segmented op: up to five 8192-token segments (csrc/hyena_longtrain.hip)
MOD_SHIFT = 0.05                             # HyenaExponentialModulation.shift
CORES = ("engine", "torch")
LONG_CORES = ("torch", "engine")
_long_read_logged = False


class HyenaTrainError(RuntimeError):
    pass


def _check(rc: int, what: str, B: int, L: int):
    if rc < 0:
        raise HyenaTrainError(f"{what}(B = {B}, L = {L}): {abi_error(rc)} (include/chimeralm_hip.h)")


def _workspace_bytes(op: str, B: int, L: int) -> int:
    n = int(getattr(N.load(), f"clm_{op}_workspace_bytes")(int(B), int(L)))
    _check(n, f"clm_{op}_workspace_bytes", B, L)
    return n


def workspace_bytes(B: int, L: int) -> int:
    """Bytes of scratch one call of that shape takes (the formula of include/chimeralm_hip.h); raises for a shape the op refuses."""
    return _workspace_bytes("hyena_train", B, L)


def long_workspace_bytes(B: int, L: int) -> int:
    """The same for the segmented op (`clm_hyena_longtrain_*`, 1 <= L <= 32,769)."""
    return _workspace_bytes("hyena_longtrain", B, L)


def _checked(B: int, L: int, **tensors):
    """The op takes contiguous fp32 GPU tensors of exactly these shapes, on one device; anything else raises before a launch."""
    shapes = {"zc": (B, 3 * DM, L), "sw": (3 * DM, 3), "sb": (3 * DM,), "k": (DM, L), "D": (DM,), "c": (B, DM, L), "dy": (B, DM, L)}
    dev = tensors["zc"].device
    for name, t in tensors.items():
        if not is_plain_fp32(t, dev) or not t.is_cuda or tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name} must be a contiguous fp32 tensor {shapes[name]} on the GPU of zc, got {t.dtype} {tuple(t.shape)} "
                             f"(contiguous: {t.is_contiguous()}) on {t.device}")


def _forward(op: str, zc, sw, sb, k, D):
    if zc.dim() != 3:
        raise ValueError("zc must be [B, 768, L]")
    B, _, L = zc.shape
    _checked(B, L, zc=zc, sw=sw, sb=sb, k=k, D=D)
    ws = torch.empty(_workspace_bytes(op, B, L), dtype=torch.uint8, device=zc.device)
    c, y = torch.empty((B, DM, L), dtype=torch.float32, device=zc.device), torch.empty((B, DM, L), dtype=torch.float32, device=zc.device)
    fn = getattr(N.load(), f"clm_{op}_forward")
    _check(fn(zc.data_ptr(), sw.data_ptr(), sb.data_ptr(), k.data_ptr(), D.data_ptr(), B, L, c.data_ptr(), y.data_ptr(), ws.data_ptr(),
              stream_of(zc)), f"clm_{op}_forward", B, L)
    return c, y


def _backward(op: str, zc, sw, sb, k, D, c, dy):
    if zc.dim() != 3:
        raise ValueError("zc must be [B, 768, L]")
    B, _, L = zc.shape
    _checked(B, L, zc=zc, sw=sw, sb=sb, k=k, D=D, c=c, dy=dy)
    ws = torch.empty(_workspace_bytes(op, B, L), dtype=torch.uint8, device=zc.device)
    dzc, dsw, dsb, dk, dD = (torch.empty_like(t) for t in (zc, sw, sb, k, D))
    fn = getattr(N.load(), f"clm_{op}_backward")
    _check(fn(zc.data_ptr(), sw.data_ptr(), sb.data_ptr(), k.data_ptr(), D.data_ptr(), c.data_ptr(), dy.data_ptr(), B, L, dzc.data_ptr(),
              dsw.data_ptr(), dsb.data_ptr(), dk.data_ptr(), dD.data_ptr(), ws.data_ptr(), stream_of(zc)), f"clm_{op}_backward", B, L)
    return dzc, dsw, dsb, dk, dD


def core_forward(zc, sw, sb, k, D):
    """-> c, y [B, 256, L] of zc [B, 768, L], sw [768, 3], sb [768], k [256, L], D [256] (csrc/hyena_train.hip)."""
    return _forward("hyena_train", zc, sw, sb, k, D)


def core_backward(zc, sw, sb, k, D, c, dy):
    """-> dzc, dsw, dsb, dk, dD."""
    return _backward("hyena_train", zc, sw, sb, k, D, c, dy)


def long_core_forward(zc, sw, sb, k, D):
    """`core_forward` by the segmented op (csrc/hyena_longtrain.hip): every 1 <= L <= 32,769."""
    return _forward("hyena_longtrain", zc, sw, sb, k, D)


def long_core_backward(zc, sw, sb, k, D, c, dy):
    """`core_backward` by the segmented op."""
    return _backward("hyena_longtrain", zc, sw, sb, k, D, c, dy)


class HyenaCore(torch.autograd.Function):
    """y [B, 256, L] of zc [B, 768, L] under sw [768, 3], sb [768], k [256, L], D [256], differentiable in all five."""

    @staticmethod
    def forward(ctx, zc, sw, sb, k, D):
        args = [t.detach().float().contiguous() for t in (zc, sw, sb, k, D)]
        c, y = core_forward(*args)
        ctx.save_for_backward(*args, c)
        return y

    @staticmethod
    def backward(ctx, dy):
        zc, sw, sb, k, D, c = ctx.saved_tensors
        return core_backward(zc, sw, sb, k, D, c, dy.float().contiguous())


class HyenaLongCore(torch.autograd.Function):
    """`HyenaCore` on the segmented op: reads of up to 32,769 tokens."""

    @staticmethod
    def forward(ctx, zc, sw, sb, k, D):
        args = [t.detach().float().contiguous() for t in (zc, sw, sb, k, D)]
        c, y = long_core_forward(*args)
        ctx.save_for_backward(*args, c)
        return y

    @staticmethod
    def backward(ctx, dy):
        zc, sw, sb, k, D, c = ctx.saved_tensors
        return long_core_backward(zc, sw, sb, k, D, c, dy.float().contiguous())


def torch_core(zc, sw, sb, k, D):
    """The same operator in torch, any dtype and device: `F.conv1d` and the reference's `fftconv` at n = 2 L."""
    L = zc.shape[-1]
    uc = F.conv1d(zc, sw.unsqueeze(1), sb, padding=2, groups=zc.shape[1])[..., :L]
    x0, x1, v = uc.split(zc.shape[1] // 3, dim=1)
    g = v * x1
    n = 2 * L
    c = torch.fft.irfft(torch.fft.rfft(g, n=n) * (torch.fft.rfft(k, n=n) / n), n=n, norm="forward")[..., :L] + g * D.unsqueeze(-1)
    return c * x0


def implicit_filter(mixer, L: int) -> torch.Tensor:
    """k [256, L] of one layer's `filter_fn` (HyenaDNA `HyenaFilter.filter`), channel-major, with a graph to the filter MLP, the
    shared `freq` and `pos_emb.z[:, :L]`: z -> Linear(5, 64) -> sin(freq .) -> 2 x (Linear(64, 64) -> sin(freq .)) -> Linear(64, 256,
    no bias) -> * (exp(-t |deltas|) + 0.05)."""
    f = mixer.filter_fn
    mlp = f.implicit_filter
    freq = mlp[1].freq                                              # ONE module registered three times
    h = f.pos_emb.z[0, :L]
    for i in (0, 2, 4):
        h = torch.sin(freq * F.linear(h, mlp[i].weight, mlp[i].bias))
    k = mlp[6].weight @ h.t()                                       # [256, L]
    decay = torch.exp(-f.modulation.deltas[0, 0].abs().unsqueeze(1) * f.pos_emb.t[0, :L, 0].unsqueeze(0))
    return k * (decay + MOD_SHIFT)


def _core_for(net, L: int, device) -> str:
    global _long_read_logged
    core = net.hyena_core
    if core == "engine" and MAX_ENGINE_TOKENS < L <= MAX_LONG_TOKENS and getattr(net, "hyena_long_core", "torch") == "engine":
        core = "engine-long"
    elif core == "engine" and L > MAX_ENGINE_TOKENS:
        if not _long_read_logged:
            log.warning("chimeralm_amd: reads of %d tokens are beyond the engine's Hyena training op (%d): they train on the torch core",
                        L, MAX_ENGINE_TOKENS)
            _long_read_logged = True
        core = "torch"
    if core != "torch" and device.type != "cuda":
        raise RuntimeError('hyena_core="engine" runs on an MI355X only (move the batch to \'cuda\', or build the net with hyena_core="torch")')
    return core


def hyena_operator(net, mixer, u: torch.Tensor, core: str) -> torch.Tensor:
    """HyenaDNA `HyenaOperator.forward` of `mixer` on u [B, L, 256] (already LayerNorm-ed) -> [B, L, 256]."""
    L = u.shape[1]
    zc = torch.matmul(mixer.in_proj.weight, u.transpose(1, 2)) + mixer.in_proj.bias.unsqueeze(-1)      # [B, 768, L]
    sw, sb = mixer.short_filter.weight.squeeze(1), mixer.short_filter.bias
    k, D = implicit_filter(mixer, L), mixer.filter_fn.bias
    y = {"engine": HyenaCore.apply, "engine-long": HyenaLongCore.apply, "torch": torch_core}[core](zc, sw, sb, k, D)
    return torch.matmul(y.transpose(1, 2), mixer.out_proj.weight.t()) + mixer.out_proj.bias


def train_forward(net, input_ids: torch.Tensor) -> torch.Tensor:
    """logits [B, 2] of `net` (a `HyenaDna(trainable=True, freeze_backbone=False)` in training mode) with a graph to every parameter:
    the HyenaDNA backbone (embedding -> 4 x [LN, Hyena operator, LN, GELU-tanh MLP] -> LN) and the attention-pooling head on the
    module's own tensors.  No mask: pads count, as in the reference."""
    if input_ids.dim() != 2:
        raise ValueError("input_ids must be [batch, length]")
    bb = net.backbone.backbone
    L = input_ids.shape[1]
    core = _core_for(net, L, input_ids.device)
    net.last_train_core = core
    h = inverted_dropout(bb.embeddings.word_embeddings(input_ids.long()), net.embed_dropout, net.dropout_generator)
    for blk in bb.layers:
        r = hyena_operator(net, blk.mixer, blk.norm1(h), core) + h
        h = blk.mlp.fc2(F.gelu(blk.mlp.fc1(blk.norm2(r)), approximate="tanh")) + r
    h = bb.ln_f(h)
    att = net.head.attention
    a = torch.softmax(att[2](F.gelu(att[0](h))), dim=1)             # over ALL positions
    return head_mlp(net, (h * a).sum(dim=1))


# ------------------------------------------------------------------------------------------------------------- the loop
def fit_hyena(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 8, lr: float | None = None, seed: int = 12345,
              device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train every parameter of `model.net` (a `ClassificationLit` over `HyenaDna(trainable=True, freeze_backbone=False)`) on one GPU:
    `fit.fit` with `fit.whole_batch_step`; a batch of one read trains.  Optimizer and scheduler are the model's factories
    (ChimeraLM.new: AdamW 1e-4, weight decay 0.01, ReduceLROnPlateau); the embedding dropout follows `seed` through
    `net.dropout_generator`, the head's dropouts through torch's generator, seeded here."""
    from . import fit

    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be >= 1")
    net = model.net
    if not getattr(net, "trainable", False) or getattr(net, "freeze_backbone", False):
        raise ValueError("fit_hyena trains HyenaDna(trainable=True, freeze_backbone=False); the head alone is headtrain.fit_head")
    torch.manual_seed(int(seed))                                     # the head's dropout masks
    return fit.fit(model, train_rows, val_rows, out_dir, params=fit.trainable_parameters(net, "net"), step=fit.whole_batch_step,
                   min_reads=1, config="lm.ChimeraLM.new", epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device,
                   tokenizer=tokenizer, metrics_factory=metrics_factory)
