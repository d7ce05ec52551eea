"""Fine-tune the Hyena head on labelled reads with the backbone frozen (the reference's `HyenaDna(freeze_backbone=True)` under
`train.py`; /root/reference/chimeralm/models/components/hyena.py:218-256, basic_module.py `training_step`).

The backbone runs in the engine exactly as in inference and leaves the final residual rows on the device (`Engine.rows`).  The one
part of the head that sees L tokens per read, the attention pooling, runs forward and backward in the engine on the module's CURRENT
`head.attention.{0,2}` parameters (csrc/pool_train.hip, `clm_pool_forward` / `clm_pool_backward`), wrapped here as a
`torch.autograd.Function`; the classifier behind it sees one 256-vector per read and is plain torch on the module's own `nn.Linear`s.

Deliberate difference from the reference: the frozen backbone runs in INFERENCE arithmetic.  The reference leaves the backbone's
embedding dropout (0.1) active while frozen, because `freeze_backbone` only clears `requires_grad`; here no backbone dropout exists
(DESIGN.md).  The head's own dropouts follow `module.training`, as in the reference.
"""
from __future__ import annotations

import torch

from ._reload import reload_signature

TRAIN_PRECISIONS = ("fp32", "fp16x3")                    # the arithmetics whose kernels leave the fp32 rows (clm_rows)


def check_train_precision(precision: str) -> None:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"the head trains on the rows of the exact kernels: precision must be 'fp32' or 'fp16x3', not {precision!r}")


class AttentionPool(torch.autograd.Function):
    """pooled [B, 256] = attention pooling of `rows` [B, L, 256] under (w1, b1, w2, b2), differentiable in those four.  `generation`
    is `Engine.rows_generation()` at the time the rows were taken from the engine's workspace (None: the caller owns `rows`);
    `backward` raises, before anything is launched, if the engine has run since: stale rows must not be read."""

    @staticmethod
    def forward(ctx, eng, rows, generation, w1, b1, w2, b2):
        w1c, b1c, w2c = w1.detach().contiguous(), b1.detach().contiguous(), w2.detach().contiguous()
        scores, stats, pooled = eng.pool_forward(rows, w1c, b1c, w2c.view(-1), b2.detach().contiguous())
        ctx.eng, ctx.rows, ctx.generation = eng, rows, generation
        ctx.w2_shape, ctx.b2_shape = w2.shape, b2.shape
        ctx.save_for_backward(w1c, b1c, w2c, scores, stats, pooled)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        eng = ctx.eng
        if ctx.generation is not None and eng.rows_generation() != ctx.generation:
            raise RuntimeError("the engine ran another forward (or reloaded its weights) since this graph's forward: the residual rows "
                               "it would differentiate through are gone.  Call backward() before the next forward")
        w1, b1, w2, scores, stats, pooled = ctx.saved_tensors
        d_w1, d_b1, d_w2, d_b2 = eng.pool_backward(ctx.rows, w1, b1, w2.view(-1), scores, stats, pooled, dpooled.contiguous())
        return None, None, None, d_w1, d_b1, d_w2.view(ctx.w2_shape), d_b2.view(ctx.b2_shape)


def train_engine(net, device: torch.device):
    """The module's engine for the frozen-backbone forward: reloaded when a BACKBONE tensor changed, not when the optimizer moved the
    head -- the engine's own copy of the head is not used here (its logits are discarded).  The next inference forward sees the
    full signature differ and reloads everything, as always."""
    sig = reload_signature(net.backbone)
    eng = getattr(net, "_engine", None)
    if eng is None or eng.device != device or getattr(net, "_backbone_sig", None) != sig:
        eng = net.engine(device)
        net._backbone_sig = sig
    return eng


def head_mlp(net, pooled: torch.Tensor) -> torch.Tensor:
    """classifier + output_layer of the reference head (hyena.py:134-146) as the torch modules they are; dropout follows training."""
    head = net.head
    c = head.classifier
    x = c[2](c[1](c[0](pooled)))
    x = c[5](c[4](c[3](x)))
    res = c[6]
    x = res.dropout(res.layers(x)) + x                   # ResidualBlock (hyena.py:160-180)
    return head.output_layer(x)


def differentiable_logits(net, input_ids: torch.Tensor) -> torch.Tensor:
    """logits [B, 2] with a graph to the head's parameters.  The batch goes through the engine in micro-batches of at most one chunk
    of reads; the rows of every micro-batch but the last are copied out of the engine's workspace (the next forward rewrites it),
    the last one's are read in place -- so one `backward()` serves the whole batch, and must come before the next forward."""
    check_train_precision(net.precision)
    if input_ids.device.type != "cuda":
        raise RuntimeError("chimeralm_amd.HyenaDna runs on an MI355X only (move the batch to 'cuda'); there is no CPU forward")
    eng = train_engine(net, input_ids.device)
    B, L = input_ids.shape
    step = eng.chunk_reads_for(L)                        # reads the engine runs as ONE chunk: the micro-batch
    att0, att2 = net.head.attention[0], net.head.attention[2]
    out = []
    for b0 in range(0, B, step):
        eng.forward(input_ids[b0:b0 + step])              # (the engine's own logits -- its copy of the head -- are discarded)
        rows, gen = eng.rows(), eng.rows_generation()
        if b0 + step < B:
            rows, gen = rows.clone(), None
        pooled = AttentionPool.apply(eng, rows, gen, att0.weight, att0.bias, att2.weight, att2.bias)
        out.append(head_mlp(net, pooled))
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)


# ------------------------------------------------------------------------------------------------------------- the loop
def head_parameters(model) -> list[torch.nn.Parameter]:
    return [p for p in model.net.head.parameters() if p.requires_grad]


def fit_head(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 16, lr: float | None = None,
             seed: int = 12345, device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train `model.net.head` (a `ClassificationLit` over `HyenaDna(freeze_backbone=True)`) on one GPU: `fit.fit` over the head's
    parameters (the reference's AdamW 1e-4 / 0.01 and ReduceLROnPlateau) with `fit.micro_batch_step` -- a batch runs as micro-batches
    of one engine chunk whose losses are plain cross-entropy shares of the batch's mean (`model.criterion` is not consulted), and no
    short last batch is skipped.  The head's dropout masks follow torch's generator, seeded here."""
    from . import fit

    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be >= 1")
    params = head_parameters(model)
    if not params:
        raise ValueError("the head has no trainable parameter")
    torch.manual_seed(seed)                                   # the head's dropout masks
    return fit.fit(model, train_rows, val_rows, out_dir, params=params, step=fit.micro_batch_step, min_reads=1, config="lm.ChimeraLM.new",
                   epochs=epochs, batch_size=batch_size, lr=lr, seed=seed, device=device, tokenizer=tokenizer, metrics_factory=metrics_factory)
