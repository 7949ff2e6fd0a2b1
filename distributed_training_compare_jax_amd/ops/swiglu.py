"""SwiGLU MLP (``ModelConfig.mlp: swiglu``; the gated MLP of the Llama / Mistral / Qwen families)::

    g = x·Wgᵀ + bg      u = x·Wuᵀ + bu      h = silu(g) ⊙ u      y = h·W2ᵀ + b2

``fc1.w`` is ``[2F, D]``, gate rows then up rows, so ``gu = x·fc1.wᵀ + fc1.b`` is ``[M, 2F]`` = ``g | u``; it is what the
backward keeps.  GPU paths (``csrc/swiglu.hip``), recorded per call in :data:`LAST` as ``attention.attn_plan`` records
its launches:

* ``fused``: one dual-panel MFMA launch for the forward (``glu_fwd_kernel``: ``gu`` and ``h`` from the fp32
  accumulators) and one for the fc2 dgrad with the gate backward in its epilogue (``glu_bwd_kernel``, on the transposed
  fc2 mirror).  bf16, ``F % 64 == 0``, ``D % 64 == 0``, 16-byte aligned rows; by default up to ``D = 1024``, where it
  was measured not slower than the unfused path (:data:`FUSE_MAX_K`).
* ``unfused``: an ordinary GEMM with an fp32 output (``gu`` at ``N = 2F``, or ``dh = dy·W2``) and an elementwise kernel
  behind it; ``h`` / ``dgu`` come from fp32 values on both paths, so both meet the same bounds (docs/NUMERICS.md).
  It serves ``dtype: fp32``, shapes outside the contract, wide models, a missing transposed mirror and
  ``DTC_SWIGLU_FUSE=0``.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import _native as N
from . import gemm as G

BH, BK = 64, 64  # hidden units / k-step of a fused tile (csrc/swiglu.hip)
# DTC_SWIGLU_FUSE=1 (default) takes the fused pair up to this K = d_model: in the step it is 0.23 ms (2.0 %) faster than
# the unfused path at d_model 768 and 2.4 ms (1.5 %) slower at 2048, where the ordinary GEMMs run their 256^2 tiles
# (profiles/swiglu.md); nothing between the two was timed.  DTC_SWIGLU_FUSE=2 takes it wherever the contract holds.
FUSE_MAX_K = 1024
LAST = {"fc1": None, "fc2_dgrad": None}  # "fused" | "unfused" | "torch": what served the last call


def swiglu_act(gu: torch.Tensor, out_dtype: Optional[torch.dtype] = None):
    """``(gu in out_dtype, h = silu(g) ⊙ u)`` from ``gu = g | u`` ``[M, 2F]`` (bf16 or fp32; fp32 arithmetic)."""
    M, F = gu.shape[0], gu.shape[1] // 2
    out_dtype = out_dtype or gu.dtype
    if not gu.is_cuda:
        g, u = gu.float().split(F, 1)
        return gu.to(out_dtype), (g * torch.sigmoid(g) * u).to(out_dtype)
    assert gu.is_contiguous() and F % 4 == 0 and (gu.dtype, out_dtype) in (
        (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32), (torch.float32, torch.bfloat16))
    h = torch.empty(M, F, dtype=out_dtype, device=gu.device)
    mode = 0 if gu.dtype == torch.bfloat16 else (1 if out_dtype == torch.float32 else 2)
    gu_out = torch.empty(M, 2 * F, dtype=out_dtype, device=gu.device) if mode == 2 else None
    N.check(N.lib().dtc_swiglu_fwd(gu.data_ptr(), N.ptr(gu_out), h.data_ptr(), mode, M, F, N.stream_ptr(gu.device)),
            "dtc_swiglu_fwd")
    return (gu if gu_out is None else gu_out), h


def swiglu_act_bwd(dh: torch.Tensor, gu: torch.Tensor) -> torch.Tensor:
    """``dgu = [dh ⊙ u ⊙ σ(g)(1 + g(1 − σ(g))) | dh ⊙ g·σ(g)]`` (the dtype of ``gu``) from fp32 ``dh`` ``[M, F]``."""
    M, F = dh.shape
    if not dh.is_cuda:
        g, u = gu.float().split(F, 1)
        s = torch.sigmoid(g)
        dhf = dh.float()
        return torch.cat([dhf * u * s * (1 + g * (1 - s)), dhf * g * s], 1).to(gu.dtype)
    assert dh.dtype == torch.float32 and dh.is_contiguous() and gu.is_contiguous() and F % 4 == 0
    dgu = torch.empty_like(gu)
    N.check(N.lib().dtc_swiglu_bwd(dh.data_ptr(), gu.data_ptr(), dgu.data_ptr(), 1 if gu.dtype == torch.float32 else 0,
                                   M, F, N.stream_ptr(dh.device)), "dtc_swiglu_bwd")
    return dgu


def _fusable(a: torch.Tensor, b: torch.Tensor, F: int) -> bool:
    """The fused pair's support contract for the GEMM operands ``a`` [M, K] and ``b`` [rows, K]."""
    knob = os.environ.get("DTC_SWIGLU_FUSE", "1")
    K = a.shape[1]
    if knob not in ("1", "2") or (knob == "1" and K > FUSE_MAX_K) or a.dtype != b.dtype or a.dtype != torch.bfloat16:
        return False
    ok = lambda t: t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0  # noqa: E731
    big = max((a.shape[0] + 128) * a.stride(0), (b.shape[0] + 128) * b.stride(0)) * 2
    return F % BH == 0 and K % BK == 0 and ok(a) and ok(b) and big < (1 << 31)


def swiglu_fc1(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]):
    """``(gu, h)``: ``gu = x·wᵀ + b`` ``[M, 2F]`` and ``h = silu(g) ⊙ u`` ``[M, F]``, both in the dtype of ``x``."""
    M, K = x.shape
    F = w.shape[0] // 2
    assert w.shape == (2 * F, K)
    if not x.is_cuda:
        LAST["fc1"] = "torch"
        gu = x.float() @ w.float().t()
        if b is not None:
            gu = gu + b.float()
        return swiglu_act(gu, x.dtype)
    if _fusable(x, w, F):
        LAST["fc1"] = "fused"
        gu = torch.empty(M, 2 * F, dtype=x.dtype, device=x.device)
        h = torch.empty(M, F, dtype=x.dtype, device=x.device)
        N.check(N.lib().dtc_glu_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), N.ptr(b), gu.data_ptr(),
                                    h.data_ptr(), M, F, K, N.stream_ptr(x.device)), "dtc_glu_fwd")
        return gu, h
    LAST["fc1"] = "unfused"
    return swiglu_act(G.linear(x, w, b, out_dtype=torch.float32), x.dtype)


def swiglu_fc2_dgrad(dy: torch.Tensor, w2: torch.Tensor, w2t: Optional[torch.Tensor], gu: torch.Tensor) -> torch.Tensor:
    """``dgu`` ``[M, 2F]`` from ``dy`` ``[M, D]``, ``w2`` = fc2.w ``[D, F]`` (``w2t``: its ``[F, D]`` transposed mirror,
    or None) and the ``gu`` :func:`swiglu_fc1` returned: ``dh = dy·W2`` through the gate backward."""
    M, D = dy.shape
    F = w2.shape[1]
    if not dy.is_cuda:
        LAST["fc2_dgrad"] = "torch"
        return swiglu_act_bwd(dy.float() @ w2.float(), gu)
    if w2t is not None and _fusable(dy, w2t, F) and gu.dtype == torch.bfloat16 and gu.is_contiguous():
        LAST["fc2_dgrad"] = "fused"
        dgu = torch.empty_like(gu)
        N.check(N.lib().dtc_glu_bwd(dy.data_ptr(), dy.stride(0), w2t.data_ptr(), w2t.stride(0), gu.data_ptr(),
                                    dgu.data_ptr(), M, F, D, N.stream_ptr(dy.device)), "dtc_glu_bwd")
        return dgu
    LAST["fc2_dgrad"] = "unfused"
    dh = G.linear(dy, w2t, out_dtype=torch.float32) if w2t is not None else G.matmul_nn(dy, w2)
    return swiglu_act_bwd(dh, gu)
