"""Rotary position embeddings (RoPE), rotate-half pairing (Llama / GPT-NeoX).

Within each Q and K head of the packed ``qkv`` activation, element ``i < hd/2`` pairs with ``i + hd/2`` and the pair is
rotated by the angle ``t * theta**(-2i/hd)`` of its position ``t``::

    lo' = lo * cos[t, i] - hi * sin[t, i]
    hi' = hi * cos[t, i] + lo * sin[t, i]

Only position DIFFERENCES reach the attention scores (``q_t · k_s`` depends on ``t - s``), so document-masked attention
over packed rows (``TrainConfig.doc_mask_token``) is position-correct without a per-document reset.  ``inverse=True``
negates the sine: the exact transpose, which is the backward (``dq``, ``dk`` of the rotated heads → of the GEMM output).
The V columns are never touched.

GPU path: ``csrc/rope.hip`` (in place, fp32 math, one rounding to the tensor's dtype).  The CPU path below does the same
fp32 arithmetic in torch.  Not implemented: the interleaved (GPT-J) pairing, partial rotary dimensions, position
offsets (KV-cache decode), NTK / YaRN scaling.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native as N

HEAD_DIMS = (32, 64, 128)  # the kernel's instantiations (the CPU path takes any even head_dim)


def rope_table(max_seq_len: int, head_dim: int, theta: float = 10000.0, device=None) -> torch.Tensor:
    """fp32 ``[max_seq_len, head_dim / 2, 2]`` of ``(cos, sin)`` of the angles ``t * theta**(-2i/head_dim)``, which are
    computed in float64 and rounded once."""
    if head_dim < 2 or head_dim % 2:
        raise ValueError(f"rope_table: head_dim={head_dim}: expected an even head_dim")
    inv = float(theta) ** (-np.arange(0, head_dim, 2, dtype=np.float64) / head_dim)
    ang = np.arange(max_seq_len, dtype=np.float64)[:, None] * inv[None]
    tab = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
    return torch.from_numpy(tab).to(device) if device is not None else torch.from_numpy(tab)


def rope_(x: torch.Tensor, tab: torch.Tensor, n_heads: int, n_kv_heads: int, inverse: bool = False) -> torch.Tensor:
    """Rotate in place the Q and K heads of ``x [B, T, (n_heads + 2 n_kv_heads) * hd]`` (bf16 or fp32) at the positions
    ``0..T-1`` of ``tab`` (:func:`rope_table`; ``hd = 2 * tab.shape[1]``); returns ``x``.  Raises, leaving ``x`` as it
    is, for ``n_heads % n_kv_heads != 0``, ``T`` beyond the table and, on the GPU, a head_dim outside 32 / 64 / 128
    or storage that is not 16-byte aligned."""
    H, Hkv = int(n_heads), int(n_kv_heads)
    hd = 2 * tab.shape[1]
    if x.dim() != 3 or tab.dim() != 3 or tab.shape[2] != 2 or x.shape[2] != (H + 2 * Hkv) * hd:
        raise ValueError(f"rope_: x {tuple(x.shape)} is not [B, T, ({H} + 2 * {Hkv}) * {hd}] for a table "
                         f"{tuple(tab.shape)} = [positions, head_dim / 2, 2]")
    if x.dtype not in (torch.bfloat16, torch.float32) or tab.dtype != torch.float32:
        raise ValueError(f"rope_: x {x.dtype} / table {tab.dtype}: expected bf16 or fp32 activations, an fp32 table")
    if not x.is_contiguous() or not tab.is_contiguous() or tab.device != x.device:
        raise ValueError("rope_: x and the table must be contiguous and on one device")
    B, T = x.shape[0], x.shape[1]
    if N.library_path(x):
        if Hkv < 1 or H % Hkv:
            raise ValueError(f"rope_: n_heads={H} is not a multiple of n_kv_heads={Hkv}")
        if T > tab.shape[0]:
            raise ValueError(f"rope_: T={T} is beyond the table's {tab.shape[0]} positions")
        c, s = tab[:T, :, 0], tab[:T, :, 1]
        if inverse:
            s = -s
        rot = x[..., :(H + Hkv) * hd].view(B, T, H + Hkv, 2, hd // 2)
        lo, hi = rot[..., 0, :].float(), rot[..., 1, :].float()
        c, s = c[None, :, None], s[None, :, None]
        new_lo, new_hi = lo * c - hi * s, hi * c + lo * s  # both before either store (fp32: lo / hi are views of x)
        rot[..., 0, :] = new_lo.to(x.dtype)
        rot[..., 1, :] = new_hi.to(x.dtype)
        return x
    N.check(N.lib().dtc_rope(x.data_ptr(), tab.data_ptr(), B, T, H, Hkv, hd, tab.shape[0],
                             1 if x.dtype == torch.float32 else 0, 1 if inverse else 0, N.stream_ptr(x.device)),
            "dtc_rope")
    return x
