"""QK-norm (``ModelConfig.qk_norm: rmsnorm``; Qwen3 / OLMo 2 / Gemma 3): an RMSNorm over ``head_dim`` of every query and
key head of the packed ``qkv`` activation with a learned gain shared by the heads of a kind, applied before the rotary
embedding and fused with it into one in-place pass::

    rstd = rsqrt(mean_i(x_i²) + eps)      x̂ = x · rstd      z = x̂ · g       g = gq (query heads) | gk (key heads)
    y    = rope(z)   (``tab``: the table of ops/rope.py)     or    y = z    (``tab=None``: learned positions)

    dz = ropeᵀ(dy) (or dy)      dx̂ = dz · g      dx = rstd · (dx̂ − x̂ · mean_i(dx̂_i · x̂_i))
    dg[i] = β·dg[i] + Σ_rows Σ_heads dz_i · x̂_i       (query heads into dg_q, key heads into dg_k; β ∈ {0, 1})

fp32 math, one rounding to the tensor's dtype; the V columns are never touched.  The forward keeps a compact copy of the
raw Q | K columns (``qk_raw``) and ``rstd`` for the backward: ``x̂`` is rebuilt from them, never by dividing the output
by the gain.  GPU path: ``csrc/qknorm.hip`` (head_dim 32 / 64 / 128, bf16 and fp32, deterministic gain gradients
through a partial slab); the CPU path below does the same fp32 arithmetic in torch.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _native as N
from .gemm import _workspace

HEAD_DIMS = (32, 64, 128)  # the kernels' instantiations (the CPU path takes any even head_dim)


def _check(name: str, x, tab, gq, gk, H: int, Hkv: int):
    hd = gq.numel()
    if x.dim() != 3 or x.shape[2] != (H + 2 * Hkv) * hd or gk.numel() != hd:
        raise ValueError(f"{name}: x {tuple(x.shape)} is not [B, T, ({H} + 2 * {Hkv}) * {hd}] for gains of "
                         f"{gq.numel()} / {gk.numel()} elements")
    if x.dtype not in (torch.bfloat16, torch.float32) or gq.dtype != torch.float32 or gk.dtype != torch.float32:
        raise ValueError(f"{name}: x {x.dtype} / gains {gq.dtype}, {gk.dtype}: expected bf16 or fp32 activations, fp32 gains")
    if not x.is_contiguous() or not gq.is_contiguous() or not gk.is_contiguous():
        raise ValueError(f"{name}: x and the gains must be contiguous")
    if tab is not None and (tab.dim() != 3 or tab.shape[1] * 2 != hd or tab.shape[2] != 2 or tab.dtype != torch.float32
                            or not tab.is_contiguous() or tab.device != x.device):
        raise ValueError(f"{name}: table {tuple(tab.shape)} {tab.dtype}: expected a contiguous fp32 [positions, {hd // 2}, 2] "
                         "on the device of x")
    if N.library_path(x):  # what the kernel's entry point refuses
        if Hkv < 1 or H % Hkv:
            raise ValueError(f"{name}: n_heads={H} is not a multiple of n_kv_heads={Hkv}")
        if tab is not None and x.shape[1] > tab.shape[0]:
            raise ValueError(f"{name}: T={x.shape[1]} is beyond the table's {tab.shape[0]} positions")
    return hd


def _cs(tab, T: int):
    return tab[:T, :, 0][None, :, None], tab[:T, :, 1][None, :, None]  # [1, T, 1, hd/2]


def qknorm_rope_fwd_(x: torch.Tensor, tab: Optional[torch.Tensor], gq: torch.Tensor, gk: torch.Tensor, n_heads: int,
                     n_kv_heads: int, eps: float):
    """Normalise, scale and (``tab`` given) rotate in place the Q and K heads of ``x [B, T, (n_heads + 2 n_kv_heads) * hd]``
    (bf16 or fp32; ``hd = gq.numel()``).  Returns ``(x, qk_raw, rstd)``: the raw Q | K columns ``[B, T, (n_heads +
    n_kv_heads) * hd]`` in the dtype of ``x`` and the fp32 statistics ``[B, T, n_heads + n_kv_heads]``.  Raises, leaving
    ``x`` as it is, for ``n_heads % n_kv_heads != 0``, ``T`` beyond the table and, on the GPU, a head_dim outside
    32 / 64 / 128 or storage that is not 16-byte aligned."""
    H, Hkv = int(n_heads), int(n_kv_heads)
    hd = _check("qknorm_rope_fwd_", x, tab, gq, gk, H, Hkv)
    B, T, nrot = x.shape[0], x.shape[1], H + Hkv
    if N.library_path(x):
        qk = x[..., :nrot * hd]
        raw = qk.clone()
        xf = qk.float().view(B, T, nrot, hd)
        rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
        g = torch.cat([gq.expand(H, hd), gk.expand(Hkv, hd)], 0)
        z = xf * rstd[..., None] * g
        if tab is not None:
            c, s = _cs(tab, T)
            lo, hi = z[..., :hd // 2], z[..., hd // 2:]
            z = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)
        qk.copy_(z.view(B, T, nrot * hd))
        return x, raw, rstd
    raw = torch.empty(B, T, nrot * hd, dtype=x.dtype, device=x.device)
    rstd = torch.empty(B, T, nrot, dtype=torch.float32, device=x.device)
    N.check(N.lib().dtc_qknorm_fwd(x.data_ptr(), N.ptr(tab), gq.data_ptr(), gk.data_ptr(), raw.data_ptr(), rstd.data_ptr(),
                                   B, T, H, Hkv, hd, 0 if tab is None else tab.shape[0], float(eps),
                                   1 if x.dtype == torch.float32 else 0, N.stream_ptr(x.device)), "dtc_qknorm_fwd")
    return x, raw, rstd


def qknorm_rope_bwd_(dy: torch.Tensor, tab: Optional[torch.Tensor], qk_raw: torch.Tensor, rstd: torch.Tensor,
                     gq: torch.Tensor, gk: torch.Tensor, n_heads: int, n_kv_heads: int, dg_q: torch.Tensor,
                     dg_k: torch.Tensor, beta: float = 0.0, red=None) -> torch.Tensor:
    """The backward of :func:`qknorm_rope_fwd_`, in place on the Q | K columns of ``dy`` (``dqkv`` as the attention
    backward left it; the V columns stay); ``qk_raw`` / ``rstd`` are the forward's.  Writes ``dg_q`` / ``dg_k`` (fp32
    ``[hd]``) ``= β·dg + Σ_rows Σ_heads dz·x̂`` (β ∈ {0, 1}); ``red``: a ``GradReducer`` that finishes the partials in its
    batched launch (bitwise the direct reduction).  Returns ``dy``."""
    H, Hkv = int(n_heads), int(n_kv_heads)
    hd = _check("qknorm_rope_bwd_", dy, tab, gq, gk, H, Hkv)
    B, T, nrot = dy.shape[0], dy.shape[1], H + Hkv
    if qk_raw.shape != (B, T, nrot * hd) or qk_raw.dtype != dy.dtype or rstd.shape != (B, T, nrot) or \
            rstd.dtype != torch.float32 or not qk_raw.is_contiguous() or not rstd.is_contiguous():
        raise ValueError(f"qknorm_rope_bwd_: qk_raw {tuple(qk_raw.shape)} {qk_raw.dtype} / rstd {tuple(rstd.shape)} "
                         f"{rstd.dtype} are not the forward's for dy {tuple(dy.shape)} {dy.dtype}")
    if N.library_path(dy):
        qk = dy[..., :nrot * hd]
        dz = qk.float().view(B, T, nrot, hd)
        if tab is not None:  # the transposed rotation: sin -> -sin
            c, s = _cs(tab, T)
            lo, hi = dz[..., :hd // 2], dz[..., hd // 2:]
            dz = torch.cat([lo * c + hi * s, hi * c - lo * s], -1)
        xh = qk_raw.float().view(B, T, nrot, hd) * rstd[..., None]
        g = torch.cat([gq.expand(H, hd), gk.expand(Hkv, hd)], 0)
        dxh = dz * g
        dx = rstd[..., None] * (dxh - xh * (dxh * xh).mean(-1, keepdim=True))
        p = dz * xh
        for dst, v in ((dg_q, p[:, :, :H].sum((0, 1, 2))), (dg_k, p[:, :, H:].sum((0, 1, 2)))):
            dst.mul_(beta).add_(v) if beta != 0.0 else dst.copy_(v)
        qk.copy_(dx.view(B, T, nrot * hd))
        return dy
    L = N.lib()
    nbytes = int(L.dtc_qknorm_bwd_workspace_bytes(B * T, hd))
    ws = _workspace(dy.device, nbytes) if red is None else red.alloc(nbytes // 4)
    N.check(L.dtc_qknorm_bwd(dy.data_ptr(), N.ptr(tab), qk_raw.data_ptr(), rstd.data_ptr(), gq.data_ptr(), gk.data_ptr(),
                             dg_q.data_ptr(), dg_k.data_ptr(), B, T, H, Hkv, hd, 0 if tab is None else tab.shape[0],
                             1 if dy.dtype == torch.float32 else 0, 1 if beta != 0.0 else 0, ws.data_ptr(),
                             nbytes if red is not None else ws.numel(), 1 if red is not None else 0,
                             N.stream_ptr(dy.device)), "dtc_qknorm_bwd")
    if red is not None:  # partials [blocks][2][hd]: one ordered column reduction per gain
        blocks = nbytes // 4 // (2 * hd)
        for s, dst in enumerate((dg_q, dg_k)):
            red.add_tall(ws.data_ptr() + s * hd * 4, 2 * hd, blocks, dst, 1.0 if beta != 0.0 else 0.0)
    return dy
