"""Pure-torch autograd oracle of the reference GPT (fp32, no fusion, no parallelism).

A line-by-line statement of the reference semantics (``model/GPTModel.py``,
``TransformerBlock.py``, ``CausalSelfAttention.py``, ``MLP.py``,
``train/create_train_step.py:30-34``) used only by tests: the explicit fused
forward/backward of ``models/gpt.py`` (CPU path and HIP path) and every parallel layout
must agree with the gradients autograd computes here.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..config.schema import ModelConfig
from ..ops.embedding import dropout_keep_mask


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


class _FakeQuantLinear(torch.autograd.Function):
    """``deq(Q(x)) · deq(Q(bf16(W)))ᵀ`` with the e4m3 quantiser of ``ops/fp8.py``; the backward is the plain
    matmul's on the unquantised operands (straight-through)."""

    @staticmethod
    def forward(ctx, x, w, bf16_inputs, sink, mx=False):
        from ..ops import fp8 as F8
        from ..ops import mxfp8 as MX

        ctx.save_for_backward(x, w)
        x2 = x.reshape(-1, x.shape[-1])
        if bf16_inputs:
            x2 = x2.to(torch.bfloat16).float()
        if sink is not None:
            sink.append(x2.detach().clone())
        if mx:  # block scales along k (ops/mxfp8.py) for both operands
            xq = MX.dequant(MX.quant_mxfp8(x2.contiguous()))
            wq = MX.dequant(MX.quant_mxfp8(w.detach().to(torch.bfloat16).contiguous()))
        else:
            xq = F8.dequant(F8.quant_e4m3(x2.contiguous()))
            wq = F8.dequant(F8.quant_e4m3(w.detach().to(torch.bfloat16).contiguous()))
        return (xq @ wq.t()).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        return g @ w, g2.t() @ x.reshape(-1, x.shape[-1]), None, None, None


def oracle_loss(cfg: ModelConfig, params: dict, ids: torch.Tensor, labels: torch.Tensor, seed: int, step: int,
                row0: int = 0, fake_quant: bool = False, quant_bf16_inputs: bool = False,
                quant_inputs: list = None, doc_mask_token: int = -1) -> torch.Tensor:
    """Mean cross-entropy of :func:`oracle_logits` (same arguments) against ``labels``."""
    logits = oracle_logits(cfg, params, ids, seed, step, row0, fake_quant, quant_bf16_inputs, quant_inputs,
                           doc_mask_token)
    V = cfg.vocab_size
    return F.cross_entropy(logits.reshape(-1, V), labels.reshape(-1).long())


def oracle_logits(cfg: ModelConfig, params: dict, ids: torch.Tensor, seed: int, step: int,
                  row0: int = 0, fake_quant: bool = False, quant_bf16_inputs: bool = False,
                  quant_inputs: list = None, doc_mask_token: int = -1) -> torch.Tensor:
    """Logits ``[B, T, vocab_size]``.  params: name → fp32 tensor (full shapes, [out,in] Dense layout),
    requires_grad allowed.

    ``doc_mask_token`` >= 0 (``TrainConfig.doc_mask_token``): attention stops at document boundaries -- position
    ``t`` starts a document iff ``t == 0`` or ``ids[b, t-1]`` is that token, and a query sees only the keys of its own
    document up to itself.

    ``fake_quant`` (default off): the four layer GEMMs of every block (qkv, out_proj, fc1, fc2) run as
    :class:`_FakeQuantLinear`, the statement of ``TrainConfig.fwd_gemm_dtype: fp8``; the lm_head stays as it is.
    ``quant_bf16_inputs`` rounds each quantiser's activation input to bf16 first (what the bf16 engine feeds it);
    ``quant_inputs``: a list that collects every quantiser's activation input, in call order.
    ``fake_quant="mx"``: the same with the MXFP8 quantiser of ``ops/mxfp8.py`` (one scale per 32 elements of k), the
    statement of ``fwd_gemm_dtype: mxfp8``."""
    if fake_quant not in (False, True, "mx"):
        raise ValueError(f"fake_quant={fake_quant!r}: expected False, True or 'mx'")
    if fake_quant:
        mx = fake_quant == "mx"
        mm = lambda a, w: _FakeQuantLinear.apply(a, w, quant_bf16_inputs, quant_inputs, mx)  # noqa: E731
    else:
        mm = lambda a, w: a @ w.t()  # noqa: E731
    B, T = ids.shape
    D, H = cfg.d_model, cfg.n_heads
    hd = D // H
    eps = cfg.layernorm_eps
    h = params["wte"][ids.long()] + params["wpe"][:T][None]
    if cfg.dropout > 0:
        keep = dropout_keep_mask(B * T, D, row0 * T, cfg.dropout, seed, step).view(B, T, D).to(h.device)
        h = torch.where(keep, h / (1 - cfg.dropout), torch.zeros_like(h))
    mask = torch.tril(torch.ones(T, T, device=h.device))
    add_mask = torch.where(mask == 1, 0.0, -1e9)  # GPTModel.py:50-51
    if doc_mask_token >= 0:  # [B, 1, T, T]: the same additive form, keys before the query's document masked too
        started = torch.ones(B, T, dtype=torch.bool, device=h.device)
        started[:, 1:] = ids[:, :-1] == doc_mask_token
        pos = torch.arange(T, device=h.device)
        doc_start = torch.cummax(torch.where(started, pos.expand(B, T), torch.full((B, T), -1, device=h.device)), 1).values
        see = (pos[None, None, :] >= doc_start[:, :, None]) & (mask == 1)[None]
        add_mask = torch.where(see, 0.0, -1e9)[:, None]
    for l in range(cfg.n_layers):
        p = lambda n: params[f"h.{l}.{n}"]  # noqa: E731
        r = h
        x = F.layer_norm(h, (D,), p("ln1.g"), p("ln1.b"), eps)
        qkv = mm(x, p("qkv.w")) + p("qkv.b")
        q, k, v = qkv.view(B, T, 3, H, hd).unbind(2)
        s = torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5 + add_mask
        a = torch.softmax(s, -1)
        o = torch.einsum("bhts,bshd->bthd", a, v).reshape(B, T, D)
        h = mm(o, p("out.w")) + p("out.b") + r
        r = h
        x = F.layer_norm(h, (D,), p("ln2.g"), p("ln2.b"), eps)
        x = _gelu_tanh(mm(x, p("fc1.w")) + p("fc1.b"))
        h = mm(x, p("fc2.w")) + p("fc2.b") + r
    x = F.layer_norm(h, (D,), params["lnf.g"], params["lnf.b"], eps)
    V = cfg.vocab_size
    return x @ params["lm_head.w"][:V].t() + params["lm_head.b"][:V]
