"""Train SequenceCNNTransformer on one MI355X (the reference's `train.py` with `model=transformer`; the reference's
chimeralm/models/components/transformer.py in `train()`, basic_module.py `training_step`).

The attention core -- softmax(q k^T / sqrt(32)) with dropout on the probabilities, times v -- runs forward and backward in the
engine (csrc/attention_train.hip, `clm_attn_train_*`), wrapped as `AttentionCore`, a `torch.autograd.Function`.  It keeps qkv, the
output and the log-sum-exp [B, 8, L'] for the backward and nothing quadratic in the length: the probabilities are recomputed, the
dropout mask is regenerated from (seed, read, head, query, key).  Everything around it is ordinary differentiable torch on the
module's own parameters: the embedding, the Conv1d stem (as `F.linear` over shifted copies: `stem`), `pe`, the LayerNorms, in_proj / out_proj and the feed-forward (`F.linear`,
i.e. rocBLAS), the residuals, the sublayer and classifier dropouts, softmax pooling and the classifier.

The op is stateless: a net of 12 layers has 12 live autograd nodes and no rule about their order.

Deliberate differences from the reference: the attention mask comes from the op's own counter-based stream and the
other dropout masks from `net.dropout_generator`, not the reference's random stream; the training arithmetic is exact fp32 whatever
the module's inference `precision`; `nn.TransformerEncoderLayer`'s forward (post-norm, ReLU) is restated, not called.
`attention_core="torch"` swaps the op for `F.scaled_dot_product_attention` with the same `dropout_p`: the comparison path.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _native as N
from ._trainop import abi_error, inverted_dropout, stream_of

NH, HD, DM = 8, 32, 256
CORES = ("engine", "torch")
_M64 = (1 << 64) - 1


class TransformerTrainError(RuntimeError):
    pass


def workspace_bytes(B: int, L: int) -> int:
    """Bytes of scratch one backward of that shape takes (include/chimeralm_hip.h); raises for a shape the op refuses."""
    n = int(N.load().clm_attn_train_workspace_bytes(B, L))
    if n < 0:
        raise TransformerTrainError(f"clm_attn_train_workspace_bytes({B}, {L}): error {n}, {abi_error(n)}")
    return n


def layer_seed(base: int, draw: int) -> int:
    """The 64-bit seed of the `draw`-th attention call under the generator seed `base` (splitmix64 of base + (draw + 1) golden
    ratios): host arithmetic only."""
    z = (int(base) + 0x9E3779B97F4A7C15 * (int(draw) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check(rc: int, what: str, *args):
    if rc != 0:
        raise TransformerTrainError(f"{what}{args}: error {rc}, {abi_error(rc)} (include/chimeralm_hip.h: what the op refuses)")


def attention_forward(qkv: torch.Tensor, dropout_p: float, seed: int):
    """-> out [B, L, 256], lse [B, 8, L] (log2 units) of contiguous fp32 qkv [B, L, 768] on the GPU."""
    if qkv.dtype != torch.float32 or qkv.dim() != 3 or qkv.shape[2] != 3 * DM or not qkv.is_cuda:
        raise ValueError("qkv must be fp32 [B, L, 768] on the GPU")
    B, L, _ = qkv.shape
    out = torch.empty((B, L, DM), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, NH, L), dtype=torch.float32, device=qkv.device)
    _check(N.load().clm_attn_train_forward(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, float(dropout_p), int(seed), stream_of(qkv)),
           "clm_attn_train_forward", B, L, dropout_p)
    return out, lse


def attention_backward(qkv, out, lse, dout, dropout_p: float, seed: int) -> torch.Tensor:
    """-> dqkv [B, L, 768]."""
    B, L, _ = qkv.shape
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(workspace_bytes(B, L), dtype=torch.uint8, device=qkv.device)
    _check(N.load().clm_attn_train_backward(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
                                            B, L, float(dropout_p), int(seed), stream_of(qkv)), "clm_attn_train_backward", B, L, dropout_p)
    return dqkv


def attention_mask(B: int, L: int, dropout_p: float, seed: int, device) -> torch.Tensor:
    """keep [B, 8, L, L] uint8 of that seed: what forward and backward regenerate (tests)."""
    keep = torch.empty((B, NH, L, L), dtype=torch.uint8, device=device)
    _check(N.load().clm_attn_train_mask(keep.data_ptr(), B, L, float(dropout_p), int(seed), stream_of(keep)), "clm_attn_train_mask", B, L, dropout_p)
    return keep


class AttentionCore(torch.autograd.Function):
    """out [B, L, 256] of qkv [B, L, 768] (the raw in_proj output), differentiable in qkv.  `recorder`, when set, is called with
    (dropout_p, seed) at every forward (tests)."""

    recorder = None

    @staticmethod
    def forward(ctx, qkv, dropout_p, seed):
        x = _aligned(qkv.detach().float())
        if AttentionCore.recorder is not None:
            AttentionCore.recorder(float(dropout_p), int(seed))
        out, lse = attention_forward(x, dropout_p, seed)
        ctx.save_for_backward(x, out, lse)
        ctx.dropout_p, ctx.seed = float(dropout_p), int(seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, lse = ctx.saved_tensors
        return attention_backward(x, out, lse, _aligned(dout.float()), ctx.dropout_p, ctx.seed), None, None


def torch_core(qkv: torch.Tensor, dropout_p: float) -> torch.Tensor:
    """The same attention through `F.scaled_dot_product_attention` (its own dropout stream)."""
    B, L, _ = qkv.shape
    q, k, v = qkv.view(B, L, 3, NH, HD).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, dropout_p=float(dropout_p)).transpose(1, 2).reshape(B, L, DM)


def dropout(net, t: torch.Tensor) -> torch.Tensor:
    return inverted_dropout(t, net.dropout, net.dropout_generator)


def encoder_layer(net, layer, x: torch.Tensor) -> torch.Tensor:
    """`nn.TransformerEncoderLayer.forward` of `layer` (post-norm, ReLU, no masks) on x [B, L', 256], the attention core on the engine
    or in torch as `net.attention_core` says."""
    sa = layer.self_attn
    qkv = F.linear(x, sa.in_proj_weight, sa.in_proj_bias)
    if net.attention_core == "engine":
        a = AttentionCore.apply(qkv, float(net.dropout), net.next_attention_seed())
    else:
        a = torch_core(qkv, net.dropout)
    x = layer.norm1(x + dropout(net, sa.out_proj(a)))
    f = layer.linear2(dropout(net, F.relu(layer.linear1(x))))
    return layer.norm2(x + dropout(net, f))


def stem(net, x: torch.Tensor) -> torch.Tensor:
    """`net.cnn` (three times Conv1d(k = 3, padding 1) -> ReLU -> MaxPool1d(2)) on channels-last x [B, L, 256] -> [B, L // 8, 256], each
    convolution as ONE `F.linear` over the three shifted copies of its input: torch's Conv1d on this stack is not run-to-run
    deterministic (identical calls differed by 5e-7 in the stem's output, measured), rocBLAS's sgemm is."""
    for i in (0, 3, 6):
        conv = net.cnn[i]
        xp = F.pad(x, (0, 0, 1, 1))
        taps = torch.cat([xp[:, :-2], xp[:, 1:-1], xp[:, 2:]], dim=-1)                # [B, L, 3 C]: tap k = x[t + k - 1]
        w = conv.weight.permute(0, 2, 1).reshape(conv.out_channels, -1)              # [out, in, k] -> [out, k * in]
        x = F.relu(F.linear(taps, w, conv.bias))
        n = x.shape[1] // 2
        x = torch.maximum(x[:, 0:2 * n:2], x[:, 1:2 * n:2])                            # MaxPool1d(2, 2): floors
    return x


def train_forward(net, input_ids: torch.Tensor) -> torch.Tensor:
    """logits [B, 2] of `net` (a `SequenceCNNTransformer(trainable=True)` in training mode) with a graph to every parameter: the
    reference's forward statement (transformer.py:82-100)."""
    x = net.embedding(input_ids.long())
    x = stem(net, x)
    Lp, max_len = x.shape[1], net.pos_encoder.pe.shape[1]
    if Lp < 1 or Lp > max_len:
        raise ValueError(f"{input_ids.shape[1]} tokens give {Lp} positions; the net takes 1 ... {max_len} (8 ... {8 * max_len + 7} tokens)")
    x = net.norm(x + net.pos_encoder.pe[:, :Lp])
    for layer in net.transformer_encoder.layers:
        x = encoder_layer(net, layer, x)
    w = torch.softmax(net.attn_pool(x), dim=1)
    pooled = torch.sum(w * x, dim=1)
    c = net.classifier
    return c[3](dropout(net, c[1](c[0](pooled))))


# ------------------------------------------------------------------------------------------------------------- the loop
def fit_transformer(model, train_rows, val_rows, out_dir, *, epochs: int = 10, batch_size: int = 8, lr: float | None = None,
                    seed: int = 12345, device: torch.device | str = "cuda", tokenizer=None, metrics_factory=None) -> list[dict]:
    """Train every parameter of `model.net` (a `ClassificationLit` over `SequenceCNNTransformer(trainable=True)`) on one GPU:
    `fit.fit` with `fit.whole_batch_step` -- nothing here couples the reads of a batch, so a batch of one read trains.  Optimizer and
    scheduler are the model's factories (configs/model/transformer.yaml: AdamW 1e-4, weight decay 0.01, ReduceLROnPlateau); the
    dropout masks and the attention seeds follow `seed` through `net.dropout_generator`."""
    from . import fit

    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be >= 1")
    torch.manual_seed(int(seed))                                     # (the torch core's dropout stream)
    return fit.fit(model, train_rows, val_rows, out_dir, params=fit.trainable_parameters(model.net, "net"), step=fit.whole_batch_step,
                   min_reads=1, config="configs/model/transformer.yaml", epochs=epochs, batch_size=batch_size, lr=lr, seed=seed,
                   device=device, tokenizer=tokenizer, metrics_factory=metrics_factory)
