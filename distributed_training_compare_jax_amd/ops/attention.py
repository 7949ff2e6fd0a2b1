"""Causal multi-head self-attention core.

Reference: ``model/CausalSelfAttention.py:34-44`` — ``softmax(QKᵀ·hd^-½ + mask)·V`` with an
additive ``-1e9`` causal mask (``model/GPTModel.py:50-51``) and the full ``[B,H,T,T]`` fp32
score tensor materialised.  Here the mask is an in-kernel predicate (``-1e9`` then ``exp``
is exactly 0 in fp32, so the semantics are identical) and the scores never leave the chip:
``csrc/attention.hip`` is a flash-style kernel (online softmax, LSE saved for backward,
P recomputed in backward) for head_dim 32, 64 and 128: ``mfma_f32_16x16x32_bf16`` kernels resident in LDS
at head_dim 32 (= one MFMA K), ``mfma_f32_32x32x16_bf16`` kernels with 32 queries or keys per wave at head_dim
64 and 128.  Any other head_dim raises ``NotImplementedError`` before anything is launched.
fp32 tensors (the exact-fp32 parity mode) run ``csrc/attention_f32.hip``: the same algorithm on
``v_mfma_f32_32x32x2_f32`` (exact f32), again with no ``[B,H,T,T]`` tensor anywhere.

Layout: the fused QKV GEMM writes ``qkv[B, T, 3, H, hd]`` (bf16); attention reads Q/K/V
in place with strides and writes ``o[B, T, H, hd]`` which is directly the out_proj input.

Which bf16 kernels a call runs is decided in one place, ``csrc/attn_plan.h``: ``plan_attn_fwd`` / ``plan_attn_bwd``
map (B, T, H, head_dim, flags, CU count, the ``DTC_ATTN_*`` knobs) to a path, its launches (kernel, grid, block,
LDS bytes) and the block order, and ``dtc_attn_fwd`` / ``dtc_attn_bwd`` launch from that plan.  :func:`plan_fwd` /
:func:`plan_bwd` ask the same plan without launching, and :func:`last_launch` reads the record the launch site
wrote, so a test can assert which kernels a shape reached.  :class:`FwdFlags` / :class:`BwdFlags` name the A/B bits.

Document-masked attention (packed sequences): :func:`doc_bounds` turns ``ids[B, T]`` and a separator id into
``(doc_start, doc_end)`` (int32 ``[B, T]``) and ``attn_fwd`` / ``attn_bwd`` take them as ``doc=``: query ``q`` sees
key ``k`` iff ``doc_start[b, q] <= k <= q``, equivalently ``k <= q < doc_end[b, k]``.  On the GPU that is the
doc instantiations of the 32-row kernels at head_dim 64 and 128, bf16 (any other head_dim is refused with code
4005, fp32 tensors raise ``NotImplementedError``); on the CPU a materialised boolean mask, any head_dim.
"""

from __future__ import annotations

import collections
import ctypes
import enum

import torch

from . import _native as N
from .gemm import _workspace


class FwdFlags(enum.IntFlag):
    """A/B switches of one :func:`attn_fwd` call (``ap::FwdFlags`` in ``csrc/attn_plan.h``)."""
    PLAIN_WAVES = 1    # resident kernel (head_dim 32): plain wave → query-group order
    CHUNK16 = 4        # head_dim 64: the 16-row chunk kernel
    ROUND4 = 16        # head_dim 64: the round-4 32-row kernel
    WPS2 = 32          # head_dim 64: the round-5 pipeline at 2 waves per SIMD (the default runs it at 3)
    HEAVY_FIRST = 64   # head_dim 64: the round-5 pipeline in heavy-first block order, not CU-balanced


class BwdFlags(enum.IntFlag):
    """A/B switches of one :func:`attn_bwd` call (``ap::BwdFlags`` in ``csrc/attn_plan.h``)."""
    TWO_ROUND = 1      # resident kernels (head_dim 32): the two-round kernels, not the fused single round
    CHUNK16 = 4        # head_dim 64: the 16-row chunk kernels
    FORCE_MERGED = 8   # head_dim 64: the merged dK/dV + dQ launch even with DTC_ATTN_BWD_MERGED=0


# enums of csrc/attn_plan.h as names, in its order (last_launch checks the counts once; tests/test_attn_plan_cpu.py
# holds the kernel names to the header's own table)
DIRECTIONS = ("none", "fwd", "bwd")
ORDERS = ("none", "heavy_first", "balanced")
PATHS = ("none", "fwd_resident", "fwd_pipe3", "fwd_pipe2", "fwd_rows32", "fwd_chunk", "fwd_tiled", "bwd_res_fused",
         "bwd_res_split", "bwd_res_merged", "bwd_rows32_128", "bwd_rows32_merged", "bwd_rows32_split", "bwd_chunk",
         "bwd_tiled", "fwd_rows32_doc", "bwd_rows32_doc_128", "bwd_rows32_doc_merged")
KERNELS = ("none", "attn_delta_kernel<32>", "attn_delta_kernel<64>", "attn_delta_kernel<128>", "attn_fwd_kernel<32>",
           "attn_fwd_kernel<64>", "attn_fwd_res_kernel<32>", "attn_fwd_chunk_kernel<32>", "attn_fwd_chunk_kernel<64>",
           "attn_fwd32_kernel<64>", "attn_fwd32_kernel<128>", "attn_fwd5_kernel<64,2>", "attn_fwd5_kernel<64,3>",
           "attn_bwd_dkdv_kernel<32>", "attn_bwd_dkdv_kernel<64>", "attn_bwd_dq_kernel<32>", "attn_bwd_dq_kernel<64>",
           "attn_bwd_fused_kernel<32>", "attn_bwd_dkdv_res_kernel<32>", "attn_bwd_dq_res_kernel<32>",
           "attn_bwd_res_kernel<32>", "attn_bwd_dq_chunk_kernel<32>", "attn_bwd_dq_chunk_kernel<64>",
           "attn_bwd_dkdv_chunk_kernel<32>", "attn_bwd_dkdv_chunk_kernel<64>", "attn_bwd_dq32_kernel<64>",
           "attn_bwd_dq32_kernel<128,true>", "attn_bwd_dkdv32_kernel<64>", "attn_bwd_dkdv32_kernel<128>",
           "attn_bwd_merged32_kernel<64>", "attn_fwd32_doc_kernel<64>", "attn_fwd32_doc_kernel<128>",
           "attn_bwd_dq32_doc_kernel<128>", "attn_bwd_dkdv32_doc_kernel<128>", "attn_bwd_merged32_doc_kernel<64>")
REC_INTS = 17
_ENUMS_CHECKED = [False]

Launch = collections.namedtuple("Launch", "kernel grid block lds")


class AttnLaunch(collections.namedtuple("AttnLaunch", "direction path order order_n launches")):
    """``direction`` fwd / bwd, ``path`` (one of :data:`PATHS`), the block ``order`` asked of ``attn_fwd5<64,3>``
    (one of :data:`ORDERS`; ``order_n`` = blocks per XCD of the balanced order, 0 when the grid is not one round
    and the kernel runs heavy-first after all) and the ``launches`` in order, each a :class:`Launch` with the
    kernel's name (one of :data:`KERNELS`), grid, block and dynamic LDS bytes."""
    __slots__ = ()

    @property
    def kernels(self):
        return tuple(l.kernel for l in self.launches)


def _record(out) -> AttnLaunch:
    v = list(out)
    launches = tuple(Launch(KERNELS[v[5 + 4 * i]], *v[6 + 4 * i:9 + 4 * i]) for i in range(v[4]))
    return AttnLaunch(DIRECTIONS[v[0]], PATHS[v[1]], ORDERS[v[2]], v[3], launches)


def _rec_buffer():
    if not _ENUMS_CHECKED[0]:
        L = N.lib()
        assert (L.dtc_attn_kernel_count(), L.dtc_attn_path_count(), L.dtc_attn_rec_ints()) == (
            len(KERNELS), len(PATHS), REC_INTS)
        _ENUMS_CHECKED[0] = True
    return (ctypes.c_int * REC_INTS)()


def last_launch() -> AttnLaunch:
    """What the last bf16 :func:`attn_fwd` / :func:`attn_bwd` of this process launched, as recorded at the launch
    site from its plan.  Tests assert it; nothing on the hot path reads it."""
    out = _rec_buffer()
    N.check(N.lib().dtc_attn_last_launch(out), "dtc_attn_last_launch")
    return _record(out)


def plan_fwd(B: int, T: int, H: int, hd: int, flags: int = 0, doc: bool = False) -> AttnLaunch:
    """The record a bf16 ``attn_fwd`` of this shape and ``flags`` would leave, without launching anything
    (``doc``: of a document-masked call).  A shape the call would refuse raises as the call does."""
    out = _rec_buffer()
    if doc:
        N.check(N.lib().dtc_attn_plan_doc(1, B, T, H, hd, int(flags), 0, out), "dtc_attn_plan_doc")
        return _record(out)
    N.check(N.lib().dtc_attn_plan(1, B, T, H, hd, int(flags), 0, out), "dtc_attn_plan")
    return _record(out)


def plan_bwd(B: int, T: int, H: int, hd: int, flags: int = 0, ws_bytes: int | None = None,
             doc: bool = False) -> AttnLaunch:
    """As :func:`plan_fwd`, for ``attn_bwd`` (``ws_bytes``: the workspace the call would hold; default: what it
    needs)."""
    L = N.lib()
    ws_bytes = int(L.dtc_attn_bwd_workspace_bytes(B, T, H, hd)) if ws_bytes is None else ws_bytes
    out = _rec_buffer()
    if doc:
        N.check(L.dtc_attn_plan_doc(2, B, T, H, hd, int(flags), ws_bytes, out), "dtc_attn_plan_doc")
        return _record(out)
    N.check(L.dtc_attn_plan(2, B, T, H, hd, int(flags), ws_bytes, out), "dtc_attn_plan")
    return _record(out)


def doc_bounds(ids: torch.Tensor, sep: int):
    """ids int32 [B, T], separator id → ``(doc_start, doc_end)``, int32 [B, T] each.  Position ``t`` starts a
    document iff ``t == 0`` or ``ids[b, t-1] == sep`` (the separator belongs to the document it ends);
    ``doc_start[b, t]`` is the largest start ``<= t``, ``doc_end[b, t]`` the smallest start ``> t``, or ``T``.
    Both are non-decreasing along ``t``.  GPU: one stream-ordered kernel (``dtc_doc_bounds``), capturable."""
    B, T = ids.shape
    if N.library_path(ids):
        pos = torch.arange(T, dtype=torch.int32, device=ids.device).expand(B, T)
        is_sep = ids == sep
        started = torch.ones(B, T, dtype=torch.bool, device=ids.device)
        started[:, 1:] = is_sep[:, :-1]
        doc_start = torch.cummax(torch.where(started, pos, torch.full_like(pos, -1)), 1).values
        nxt = torch.where(is_sep, pos + 1, torch.full_like(pos, T))  # a separator at t: t + 1 starts a document
        doc_end = torch.cummin(nxt.flip(1), 1).values.flip(1)
        return doc_start.to(torch.int32).contiguous(), doc_end.to(torch.int32).contiguous()
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    doc_start = torch.empty(B, T, dtype=torch.int32, device=ids.device)
    doc_end = torch.empty(B, T, dtype=torch.int32, device=ids.device)
    N.check(N.lib().dtc_doc_bounds(ids.data_ptr(), doc_start.data_ptr(), doc_end.data_ptr(), B, T, int(sep),
                                   N.stream_ptr(ids.device)), "dtc_doc_bounds")
    return doc_start, doc_end


def _doc_mask(doc, T: int, device) -> torch.Tensor:
    """[B, 1, T, T] boolean mask of the definition: query q sees key k iff doc_start[b, q] <= k <= q."""
    pos = torch.arange(T, device=device)
    see = (pos[None, None, :] >= doc[0].to(device).long()[:, :, None]) & (pos[None, None, :] <= pos[None, :, None])
    return see[:, None]


def _check_doc(doc, qkv):
    B, T, _ = qkv.shape
    for a in doc:
        assert a.dtype == torch.int32 and a.shape == (B, T) and a.is_contiguous() and a.device == qkv.device
    if qkv.dtype != torch.bfloat16:
        raise NotImplementedError("document-masked attention on the GPU is bf16 only (csrc/attention_f32.hip has no "
                                  "doc kernels)")


def attn_fwd(qkv: torch.Tensor, n_heads: int, scale: float | None = None, flags: int = 0, doc=None):
    """qkv [B,T,3*H*hd] → (o [B,T,H*hd], lse [B,H,T] fp32, natural-log units).  ``flags``: a :class:`FwdFlags`
    (or its integer), A/B switches of the bf16 kernels.  At head_dim 32 only ``PLAIN_WAVES`` means anything, and
    only on the resident kernel.  At head_dim 64 the default is the round-5 pipeline at 3 waves per SIMD with
    query blocks assigned to CU slots longest-processing-time-first; ``HEAVY_FIRST`` keeps that kernel in
    heavy-first order, ``WPS2`` runs it at 2 waves per SIMD, ``ROUND4`` picks the round-4 32-row kernel and
    ``CHUNK16`` the 16-row chunk kernel (``CHUNK16`` beats ``ROUND4`` beats ``WPS2``).  head_dim 128 has one
    forward kernel and ignores ``flags``.  ``doc = (doc_start, doc_end)`` (:func:`doc_bounds`): attention stops at
    document boundaries; bf16 at head_dim 64 / 128 on the GPU, whatever ``flags`` say."""
    B, T, C3 = qkv.shape
    hd = C3 // (3 * n_heads)
    scale = scale if scale is not None else hd ** -0.5
    if N.library_path(qkv):
        q, k, v = qkv.float().view(B, T, 3, n_heads, hd).unbind(2)
        s = torch.einsum("bthd,bshd->bhts", q, k) * scale
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
        if doc is not None:
            mask = _doc_mask(doc, T, qkv.device)
        s = s.masked_fill(~mask, float("-inf"))
        lse = torch.logsumexp(s, -1)
        p = torch.exp(s - lse[..., None])
        o = torch.einsum("bhts,bshd->bthd", p, v).reshape(B, T, n_heads * hd)
        return o.to(qkv.dtype), lse
    assert qkv.dtype in (torch.bfloat16, torch.float32) and qkv.is_contiguous()
    if doc is not None:
        _check_doc(doc, qkv)
        o = torch.empty(B, T, n_heads * hd, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, n_heads, T, dtype=torch.float32, device=qkv.device)
        N.check(N.lib().dtc_attn_fwd_doc(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, T, n_heads, hd, int(flags),
                                         scale, doc[0].data_ptr(), doc[1].data_ptr(), N.stream_ptr(qkv.device)),
                "dtc_attn_fwd_doc")
        return o, lse
    if hd not in (32, 64, 128):
        raise NotImplementedError(f"attention kernel supports head_dim 32/64/128, got {hd}")
    o = torch.empty(B, T, n_heads * hd, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, n_heads, T, dtype=torch.float32, device=qkv.device)
    if qkv.dtype == torch.float32:
        N.check(N.lib().dtc_attn_f32_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, T, n_heads, hd, scale,
                                         N.stream_ptr(qkv.device)), "dtc_attn_f32_fwd")
        return o, lse
    N.check(N.lib().dtc_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, T, n_heads, hd, int(flags), scale,
                                 N.stream_ptr(qkv.device)), "dtc_attn_fwd")
    return o, lse


def attn_bwd(qkv: torch.Tensor, o: torch.Tensor, lse: torch.Tensor, do: torch.Tensor, n_heads: int,
             scale: float | None = None, flags: int = 0, doc=None) -> torch.Tensor:
    """Returns dqkv [B,T,3*H*hd] (same dtype as qkv).  ``flags``: a :class:`BwdFlags` (or its integer), A/B
    switches of the bf16 kernels.  ``TWO_ROUND`` forces the two-round resident kernels instead of the fused
    single-round one (head_dim 32, resident shapes only); at head_dim 64 ``CHUNK16`` picks the 16-row chunk pair
    and ``FORCE_MERGED`` the delta pass + merged launch even with ``DTC_ATTN_BWD_MERGED=0`` (``CHUNK16`` wins).
    head_dim 128 has one backward path (delta pass, dK/dV kernel, dQ kernel) and ignores ``flags``.  ``doc``: as
    :func:`attn_fwd` (the same bounds the forward ran with); the doc kernels mirror those two paths."""
    B, T, C3 = qkv.shape
    hd = C3 // (3 * n_heads)
    scale = scale if scale is not None else hd ** -0.5
    if N.library_path(qkv):
        q, k, v = qkv.float().view(B, T, 3, n_heads, hd).unbind(2)
        dof = do.float().view(B, T, n_heads, hd)
        s = torch.einsum("bthd,bshd->bhts", q, k) * scale
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
        if doc is not None:
            mask = _doc_mask(doc, T, qkv.device)
        s = s.masked_fill(~mask, float("-inf"))
        p = torch.exp(s - lse[..., None])
        dv = torch.einsum("bhts,bthd->bshd", p, dof)
        dp = torch.einsum("bthd,bshd->bhts", dof, v)
        delta = (dof * o.float().view(B, T, n_heads, hd)).sum(-1).permute(0, 2, 1)  # [B,H,T]
        ds = p * (dp - delta[..., None]) * scale
        dq = torch.einsum("bhts,bshd->bthd", ds, k)
        dk = torch.einsum("bhts,bthd->bshd", ds, q)
        return torch.stack([dq, dk, dv], 2).reshape(B, T, C3).to(qkv.dtype)
    assert do.is_contiguous() and o.is_contiguous()
    dqkv = torch.empty_like(qkv)
    L = N.lib()
    if doc is not None:
        _check_doc(doc, qkv)
        ws = _workspace(qkv.device, int(L.dtc_attn_bwd_workspace_bytes(B, T, n_heads, hd)))
        N.check(L.dtc_attn_bwd_doc(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dqkv.data_ptr(),
                                   int(flags), B, T, n_heads, hd, scale, ws.data_ptr(), ws.numel() * ws.element_size(),
                                   doc[0].data_ptr(), doc[1].data_ptr(), N.stream_ptr(qkv.device)),
                "dtc_attn_bwd_doc")
        return dqkv
    if qkv.dtype == torch.float32:
        assert do.dtype == torch.float32 and o.dtype == torch.float32
        ws = _workspace(qkv.device, int(L.dtc_attn_f32_bwd_workspace_bytes(B, T, n_heads, hd)))
        N.check(L.dtc_attn_f32_bwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dqkv.data_ptr(), B, T,
                                   n_heads, hd, scale, ws.data_ptr(), ws.numel(), N.stream_ptr(qkv.device)),
                "dtc_attn_f32_bwd")
        return dqkv
    ws = _workspace(qkv.device, int(L.dtc_attn_bwd_workspace_bytes(B, T, n_heads, hd)))
    N.check(L.dtc_attn_bwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dqkv.data_ptr(), int(flags),
                           B, T, n_heads, hd, scale, ws.data_ptr(), ws.numel() * ws.element_size(),
                           N.stream_ptr(qkv.device)),
            "dtc_attn_bwd")
    return dqkv


def attn_flops(B: int, T: int, H: int, hd: int, causal: bool = True) -> float:
    f = 4.0 * B * H * T * T * hd
    return f / 2 if causal else f

