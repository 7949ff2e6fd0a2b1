"""RMSNorm (``ModelConfig.norm: rmsnorm``; the norm of the Llama / Mistral / Qwen / OLMo families): a learned scale, no
bias, no mean::

    rstd = rsqrt(mean(x²) + eps)        x̂ = x · rstd        y = x̂ · γ

Input is the fp32 residual stream; output is the GEMM operand dtype (bf16 on GPU).  Only ``rstd`` is saved for the
backward, which fuses the residual-gradient add (``dx = dres + rstd · (γ·dy − x̂ · mean(γ·dy·x̂))``) and emits per-block
partials of ``dγ = Σ_rows dy·x̂`` and, optionally, ``Σ_rows dx`` that are reduced deterministically (no float atomics).
GPU path: ``csrc/rmsnorm.hip`` (16-byte loads; one wave64 per row up to d_model 4096 forward / 1536 backward, a row
spread over the 4 or 8 waves of a block up to 8192; ``D % 4 == 0``).  The calls mirror ``ops/layernorm.py``.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _native as N
from .gemm import _workspace


def rmsnorm_fwd(x: torch.Tensor, g: torch.Tensor, eps: float, out_dtype: Optional[torch.dtype] = None):
    """``(y, rstd)``."""
    M, D = x.shape
    out_dtype = out_dtype or x.dtype
    if not x.is_cuda:
        xf = x.float()
        rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
        return (xf * rstd[:, None] * g.float()).to(out_dtype), rstd
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty(M, D, dtype=out_dtype, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    N.check(N.lib().dtc_rmsnorm_fwd(x.data_ptr(), g.data_ptr(), y.data_ptr(), rstd.data_ptr(), M, D, eps,
                                    1 if out_dtype == torch.float32 else 0, N.stream_ptr(x.device)), "dtc_rmsnorm_fwd")
    return y, rstd


def add_rmsnorm_fwd(d: torch.Tensor, resid: torch.Tensor, g: torch.Tensor, eps: float,
                    out_dtype: Optional[torch.dtype] = None):
    """``x = d + resid`` (fp32, written over an fp32 ``d``; a new tensor for a bf16 ``d``: ``float(d) + resid``) and
    ``(RMSNorm(x), rstd)``: the residual add of the layer that produced ``d``, done in the pass that reads the row
    anyway.  Returns ``(x, (y, rstd))``."""
    M, D = d.shape
    out_dtype = out_dtype or resid.dtype
    bf = d.dtype == torch.bfloat16
    if not d.is_cuda:
        x = d.float() + resid if bf else d.add_(resid)
        return x, rmsnorm_fwd(x, g, eps, out_dtype)
    assert d.is_contiguous() and resid.dtype == torch.float32 and resid.is_contiguous()
    assert bf or d.dtype == torch.float32
    x = torch.empty(M, D, dtype=torch.float32, device=d.device) if bf else d
    y = torch.empty(M, D, dtype=out_dtype, device=d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=d.device)
    name = "dtc_add_rmsnorm_fwd_bf16" if bf else "dtc_add_rmsnorm_fwd"
    N.check(getattr(N.lib(), name)(d.data_ptr(), resid.data_ptr(), x.data_ptr(), g.data_ptr(), y.data_ptr(),
                                   rstd.data_ptr(), M, D, eps, 1 if out_dtype == torch.float32 else 0,
                                   N.stream_ptr(d.device)), name)
    return x, (y, rstd)


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, g: torch.Tensor, rstd: torch.Tensor, dres: Optional[torch.Tensor],
                dg: torch.Tensor, beta: float = 0.0, out: Optional[torch.Tensor] = None,
                out_c: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, red=None) -> torch.Tensor:
    """Returns fp32 ``dx = dres + dRMSNorm/dx·dy``; writes ``dg = β·dg + Σ_rows dy·x̂`` (β ∈ {0, 1}).

    ``out`` may alias ``dres``; ``out_c`` (optional) receives a bf16 copy of ``dx``; ``dbias`` (optional) receives
    ``β·dbias + Σ_rows dx`` (the out_proj.b / fc2.b gradient); ``red``: a ``GradReducer`` that finishes the column
    partials in its batched launch (bitwise the direct reduction)."""
    M, D = x.shape
    if not x.is_cuda:
        xhat = x.float() * rstd[:, None]
        dyf = dy.float()
        gdy = dyf * g.float()
        dx = (gdy - xhat * (gdy * xhat).mean(-1, keepdim=True)) * rstd[:, None]
        if dres is not None:
            dx = dx + dres
        for dst, v in ((dg, (dyf * xhat).sum(0)), (dbias, dx.sum(0))):
            if dst is not None:
                dst.mul_(beta).add_(v) if beta != 0.0 else dst.copy_(v)
        if out_c is not None:
            out_c.copy_(dx)
        if out is not None:
            out.copy_(dx)
            return out
        return dx
    assert x.is_contiguous() and dy.is_contiguous()
    if out is None:
        out = torch.empty(M, D, dtype=torch.float32, device=x.device)
    L = N.lib()
    nslab = 2 if dbias is not None else 1
    nbytes = int(L.dtc_rmsnorm_bwd_workspace_bytes(M, D))
    ws = _workspace(x.device, nbytes) if red is None else red.alloc(nbytes // 4)
    N.check(L.dtc_rmsnorm_bwd(dy.data_ptr(), 1 if dy.dtype == torch.float32 else 0, x.data_ptr(), g.data_ptr(),
                              rstd.data_ptr(), N.ptr(dres), out.data_ptr(), N.ptr(out_c), dg.data_ptr(), N.ptr(dbias),
                              M, D, 1 if beta != 0.0 else 0, ws.data_ptr(), nbytes if red is not None else ws.numel(),
                              1 if red is not None else 0, N.stream_ptr(x.device)), "dtc_rmsnorm_bwd")
    if red is not None:  # partials [blocks][nslab][D]: one ordered column reduction per slab
        blocks = nbytes // 4 // (2 * D)
        for s, dst in enumerate((dg, dbias)[:nslab]):
            red.add_tall(ws.data_ptr() + s * D * 4, nslab * D, blocks, dst, 1.0 if beta != 0.0 else 0.0)
    return out
