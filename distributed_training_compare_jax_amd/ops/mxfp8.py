"""MXFP8 forward path (OCP microscaling): e4m3 bytes plus one power-of-two scale per 32 consecutive elements of k.

Quantiser (the torch CPU path below is the definition; ``csrc/gemm_fp8.hip`` ``mx_quant_tasks_kernel`` and the
producers that emit MX output beside their bf16 output agree with it bit for bit).  Input: a row-major ``[M, K]``
bf16 or fp32 tensor with ``K % 32 == 0``; block ``b`` of a row is its elements ``[32b, 32b + 32)``.  Per block:

* ``amax = max|x|`` and ``e = floor(log2(amax))``; the scale exponent is ``se = 8 - e``, or ``7 - e`` when
  ``amax·2^(8-e) > 448``, clamped to [-126, 126]; ``amax == 0`` gives ``se = 0``.  This is the per-tensor rule of
  ``ops/fp8.py`` applied per block: ``amax·2^se`` lies in (224, 448] and nothing saturates;
* ``q = RNE_e4m3(x·2^se)`` (``x·2^se`` is exact in fp32: one rounding);
* the stored scale is the E8M0 code of the dequantisation scale ``2^-se``: the byte ``127 - se`` in 1..253, in a
  row-major ``uint8 [M, K/32]`` tensor.

One pass, no atomics and no state, so the quantiser also fits inside the kernels that produce the GEMM inputs:
:func:`layernorm_fwd_mx` / :func:`add_layernorm_fwd_mx` (``d_model <= 2048``) and the GELU-pair epilogue of
:func:`linear_gelu_mxfp8` (``N % 32 == 0``) return the MX form of the bf16 tensor they store, the same bytes as
:func:`quant_mxfp8` gives on that tensor.  ``DTC_MX_FUSE=0`` sends every activation through the stand-alone
quantiser instead (an A/B and test switch, docs/KNOBS.md).

GEMMs (NT only, ``K % 128 == 0``, ``N % 16 == 0``, any ``M >= 1``; anything else raises ``NotImplementedError``
before a launch): :func:`linear_mxfp8`, :func:`linear_resid_mxfp8`, :func:`linear_gelu_mxfp8`.  The block-scaled
MFMA takes the scale bytes as they are stored; there is no scale multiply in the epilogue.  CPU tensors compute on
the dequantised operands in fp32.
"""

from __future__ import annotations

import collections
import ctypes
import os
from typing import List, Optional, Sequence

import torch

from . import _native as N
from . import layernorm as LN
from .fp8 import EPI_NAMES, QT_MAX, Fp8GemmArgs, set_tile_m  # noqa: F401  (set_tile_m: the same switch forces MX tiles)
from .gemm import gelu_tanh, gelu_tanh_grad

BLOCK = 32

# q: uint8 [M, K] (e4m3fn bytes); sc: uint8 [M, K/32] (E8M0 dequantisation scales)
MxFp8Tensor = collections.namedtuple("MxFp8Tensor", "q sc")


def fuse_enabled() -> bool:
    """``DTC_MX_FUSE`` (default 1): producers emit the MX form of their bf16 output; 0 = stand-alone quantiser."""
    return os.environ.get("DTC_MX_FUSE", "1") != "0"


class MxQuantTask(ctypes.Structure):
    """Mirror of ``struct MxQuantTask`` in csrc/gemm_fp8.hip (keep in sync)."""

    _fields_ = [("src", N.c_vp), ("q", N.c_vp), ("sc", N.c_vp), ("n32", N.c_long), ("blk0", N.c_int),
                ("nblk", N.c_int), ("f32", N.c_int), ("pad", N.c_int)]


class MxQuantBatch(ctypes.Structure):
    _fields_ = [("ntasks", N.c_int), ("nblocks", N.c_int), ("t", MxQuantTask * QT_MAX)]


class MxGemmExtra(ctypes.Structure):
    """Mirror of ``struct MxGemmExtra`` in csrc/gemm_fp8.hip (keep in sync)."""

    _fields_ = [("sa", N.c_vp), ("ldsa", N.c_long), ("sb", N.c_vp), ("ldsb", N.c_long), ("gq", N.c_vp),
                ("gsc", N.c_vp)]


# ----------------------------------------------------------------------------- quantiser
def scale_exp_from_amax(amax: torch.Tensor) -> torch.Tensor:
    """``se`` (int32) for an fp32 ``amax`` tensor of any shape, by the rule in the module docstring."""
    amax = amax.float()
    m, ex = torch.frexp(amax)  # amax = m·2^ex with m in [0.5, 1): e = ex - 1, and amax·2^(8-e) > 448 <=> m > 0.875
    se = torch.where(m > 0.875, 8 - ex, 9 - ex).clamp(-126, 126)
    return torch.where(amax > 0, se, torch.zeros_like(se)).to(torch.int32)


def _check_input(x: torch.Tensor):
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"quant_mxfp8: bf16 or fp32 input, got {x.dtype}")
    if x.dim() != 2 or not x.is_contiguous() or x.numel() == 0 or x.shape[1] % BLOCK:
        raise ValueError(f"quant_mxfp8: expected a non-empty contiguous [M, K] tensor with K % 32 == 0, got shape "
                         f"{tuple(x.shape)} strides {x.stride()}")


def _quant_cpu(x: torch.Tensor) -> MxFp8Tensor:
    M, K = x.shape
    xb = x.float().view(M, K // BLOCK, BLOCK)
    se = scale_exp_from_amax(xb.abs().amax(-1))
    q = torch.ldexp(xb, se[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).view(M, K)
    return MxFp8Tensor(q, (127 - se).to(torch.uint8))


def dequant(t: MxFp8Tensor) -> torch.Tensor:
    """fp32 values of an MX tensor: ``e4m3(q)·2^(sc - 127)`` per block (exact)."""
    M, K = t.q.shape
    v = t.q.view(torch.float8_e4m3fn).float().view(M, K // BLOCK, BLOCK)
    return torch.ldexp(v, (t.sc.to(torch.int32) - 127)[..., None]).view(M, K)


_QT_CHECKED = [False]
_BLOCK_ELEMS = 8192  # 256 threads x 4 vectors of 8 elements per block
_MAX_BLOCKS = 512    # per tensor; the kernel strides


def empty_like_mx(x: torch.Tensor) -> MxFp8Tensor:
    M, K = x.shape
    return MxFp8Tensor(torch.empty(M, K, dtype=torch.uint8, device=x.device),
                       torch.empty(M, K // BLOCK, dtype=torch.uint8, device=x.device))


def quant_mxfp8_batch(xs: Sequence[torch.Tensor], outs: Optional[Sequence[MxFp8Tensor]] = None) -> List[MxFp8Tensor]:
    """Quantise a list of tensors: one launch over a task table per chunk of :data:`QT_MAX` tensors.  ``outs``:
    preallocated outputs (a persistent mirror)."""
    xs = list(xs)
    if not xs:
        return []
    for x in xs:
        _check_input(x)
    if outs is None:
        outs = [empty_like_mx(x) for x in xs]
    outs = list(outs)
    for x, o in zip(xs, outs):
        assert o.q.dtype == torch.uint8 and o.q.is_contiguous() and tuple(o.q.shape) == tuple(x.shape)
        assert o.sc.dtype == torch.uint8 and o.sc.is_contiguous() and tuple(o.sc.shape) == (x.shape[0], x.shape[1] // BLOCK)
        assert o.q.device == x.device and o.sc.device == x.device
    if N.library_path(xs[0]):
        for x, o in zip(xs, outs):
            w = _quant_cpu(x)
            o.q.copy_(w.q)
            o.sc.copy_(w.sc)
        return outs
    dev = xs[0].device
    L = N.lib()
    if not _QT_CHECKED[0]:
        assert L.dtc_qt_max() == QT_MAX and L.dtc_mxqt_task_bytes() == ctypes.sizeof(MxQuantTask)
        assert L.dtc_mxqt_batch_bytes() == ctypes.sizeof(MxQuantBatch)
        _QT_CHECKED[0] = True
    for i0 in range(0, len(xs), QT_MAX):
        b = MxQuantBatch()
        blk = 0
        chunk = range(i0, min(i0 + QT_MAX, len(xs)))
        for j, i in enumerate(chunk):
            x, o = xs[i], outs[i]
            if x.data_ptr() % 16 or o.q.data_ptr() % 8:
                raise ValueError("quant_mxfp8: the input must be 16-byte aligned and the output 8-byte aligned")
            nblk = max(1, min(_MAX_BLOCKS, (x.numel() + _BLOCK_ELEMS - 1) // _BLOCK_ELEMS))
            b.t[j] = MxQuantTask(x.data_ptr(), o.q.data_ptr(), o.sc.data_ptr(), x.numel() // BLOCK, blk, nblk,
                                 1 if x.dtype == torch.float32 else 0, 0)
            blk += nblk
        b.ntasks, b.nblocks = len(chunk), blk
        N.check(L.dtc_quant_mxfp8_tasks(ctypes.byref(b), N.stream_ptr(dev)), "dtc_quant_mxfp8_tasks")
    return outs


def quant_mxfp8(x: torch.Tensor) -> MxFp8Tensor:
    """``(q, sc)`` of a bf16 or fp32 row-major ``[M, K]`` tensor with ``K % 32 == 0`` (see the module docstring)."""
    return quant_mxfp8_batch([x])[0]


# ----------------------------------------------------------------------------- fused producers: LayerNorm
def _ln_fusable(x: torch.Tensor, out_dtype) -> bool:
    return x.is_cuda and out_dtype == torch.bfloat16 and x.shape[1] <= 2048 and x.shape[1] % BLOCK == 0 and fuse_enabled()


def _ln_mx(x, x_bf16, resid, x_out, g, b, eps):
    M, D = x.shape
    dev = x.device
    y = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    mx = empty_like_mx(y)
    N.check(N.lib().dtc_layernorm_fwd_mx(x.data_ptr(), 1 if x_bf16 else 0, N.ptr(resid), N.ptr(x_out), g.data_ptr(),
                                         b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, D, eps,
                                         mx.q.data_ptr(), mx.sc.data_ptr(), N.stream_ptr(dev)), "dtc_layernorm_fwd_mx")
    return (y, mean, rstd), mx


def layernorm_fwd_mx(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float,
                     out_dtype: Optional[torch.dtype] = None):
    """``ops.layernorm.layernorm_fwd`` plus the MX form of ``y``: ``((y, mean, rstd), MxFp8Tensor)``.  On the GPU
    with bf16 output, ``D <= 2048`` and ``D % 32 == 0`` one kernel writes both (``y / mean / rstd`` bitwise as the
    plain call); otherwise (wide rows, CPU, ``DTC_MX_FUSE=0``) the plain LayerNorm is followed by
    :func:`quant_mxfp8` on ``y``: the same bytes."""
    out_dtype = out_dtype or x.dtype
    if not _ln_fusable(x, out_dtype):
        pre = LN.layernorm_fwd(x, g, b, eps, out_dtype)
        return pre, quant_mxfp8(pre[0])
    assert x.dtype == torch.float32 and x.is_contiguous()
    return _ln_mx(x, False, None, None, g, b, eps)


def add_layernorm_fwd_mx(d: torch.Tensor, resid: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float,
                         out_dtype: Optional[torch.dtype] = None):
    """``ops.layernorm.add_layernorm_fwd`` (fp32 or bf16 ``d``) plus the MX form of ``y``:
    ``(x, (y, mean, rstd), MxFp8Tensor)``; fused and fallback as :func:`layernorm_fwd_mx`."""
    out_dtype = out_dtype or resid.dtype
    if not _ln_fusable(d, out_dtype):
        x, pre = LN.add_layernorm_fwd(d, resid, g, b, eps, out_dtype)
        return x, pre, quant_mxfp8(pre[0])
    assert d.is_contiguous() and resid.dtype == torch.float32 and resid.is_contiguous()
    if d.dtype == torch.bfloat16:
        x = torch.empty(d.shape, dtype=torch.float32, device=d.device)
        pre, mx = _ln_mx(d, True, resid, x, g, b, eps)
        return x, pre, mx
    assert d.dtype == torch.float32
    pre, mx = _ln_mx(d, False, resid, d, g, b, eps)
    return d, pre, mx


# ----------------------------------------------------------------------------- GEMM
VARIANTS = {4: "mxfp8_128x128", 2: "mxfp8_64x128"}

LastLaunchMxFp8 = collections.namedtuple("LastLaunchMxFp8", "tile variant epilogue out_f32 blocks fused_quant")


def last_launch_mxfp8() -> LastLaunchMxFp8:
    """What the last FP8 / MXFP8 GEMM launch of this process ran, as recorded by the launch site
    (csrc/gemm_fp8.hip): ``variant`` is one of :data:`VARIANTS` for an MX kernel and one of ``ops.fp8.VARIANTS``
    for a per-tensor one; ``fused_quant``: the GELU-pair epilogue also wrote the MX form of ``gelu(u)``."""
    from .fp8 import VARIANTS as V8

    out = (ctypes.c_int * 8)()
    N.check(N.lib().dtc_gemm_fp8_last_launch(out), "dtc_gemm_fp8_last_launch")
    v = list(out)
    names = VARIANTS if v[6] else V8
    return LastLaunchMxFp8((v[0], v[1]), names.get(v[2], "none"), EPI_NAMES.get(v[3], "none"), bool(v[4]), v[5],
                           v[6] == 2)


def _check_operands(x: MxFp8Tensor, w: MxFp8Tensor):
    for t, name in ((x, "x"), (w, "w")):
        if t.q.dim() != 2 or t.q.dtype != torch.uint8 or t.q.stride(1) != 1:
            raise ValueError(f"{name}: expected row-major 2-D e4m3 bytes (uint8), got {t.q.dtype} shape "
                             f"{tuple(t.q.shape)} strides {t.q.stride()}")
        if t.sc.dtype != torch.uint8 or tuple(t.sc.shape) != (t.q.shape[0], t.q.shape[1] // BLOCK) or t.q.shape[1] % BLOCK \
                or t.sc.stride(-1) != 1:
            raise ValueError(f"{name}: expected uint8 scale bytes of shape [{t.q.shape[0]}, {t.q.shape[1]} / 32], got "
                             f"{t.sc.dtype} shape {tuple(t.sc.shape)}")
    M, K = x.q.shape
    Nn, Kw = w.q.shape
    if Kw != K:
        raise ValueError(f"linear_mxfp8: x is [{M}, {K}] but w is [{Nn}, {Kw}]")
    if M < 1 or K % 128 or K < 128 or Nn % 16 or Nn < 16:
        raise NotImplementedError(f"MXFP8 GEMM needs M >= 1, K % 128 == 0 and N % 16 == 0, got M={M} N={Nn} K={K}")
    return M, Nn, K


def _gemm_mxfp8(x: MxFp8Tensor, w: MxFp8Tensor, c: torch.Tensor, epi: int, bias, aux=None, aux_out=None,
                gq: Optional[MxFp8Tensor] = None):
    M, K = x.q.shape
    Nn = w.q.shape[0]
    if x.q.stride(0) % 16 or w.q.stride(0) % 16 or x.q.data_ptr() % 16 or w.q.data_ptr() % 16:
        raise ValueError("MXFP8 GEMM operands must be 16-byte aligned with row strides that are multiples of 16")
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Nn
    args = Fp8GemmArgs(M=M, N=Nn, K=K, A=x.q.data_ptr(), lda=x.q.stride(0), B=w.q.data_ptr(), ldb=w.q.stride(0),
                       C=c.data_ptr(), ldc=Nn, c_f32=1 if c.dtype == torch.float32 else 0, epi=epi, bias=N.ptr(bias),
                       aux=N.ptr(aux), ldaux=Nn, aux_out=N.ptr(aux_out), inv_sa=0, inv_sb=0)
    ext = MxGemmExtra(sa=x.sc.data_ptr(), ldsa=x.sc.stride(0), sb=w.sc.data_ptr(), ldsb=w.sc.stride(0),
                      gq=0 if gq is None else gq.q.data_ptr(), gsc=0 if gq is None else gq.sc.data_ptr())
    N.check(N.lib().dtc_gemm_mxfp8(ctypes.byref(args), ctypes.byref(ext), N.stream_ptr(c.device)), "dtc_gemm_mxfp8")


def _ref(x: MxFp8Tensor, w: MxFp8Tensor, bias):
    y = dequant(x) @ dequant(w).t()
    return y if bias is None else y + bias.float()


def linear_mxfp8(x: MxFp8Tensor, w: MxFp8Tensor, bias: Optional[torch.Tensor] = None,
                 out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``y = deq(x)·deq(w)ᵀ + b`` (bf16 or fp32 out)."""
    M, Nn, _ = _check_operands(x, w)
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"linear_mxfp8: bf16 or fp32 output, got {out_dtype}")
    if N.library_path(x.q):
        return _ref(x, w, bias).to(out_dtype)
    y = torch.empty(M, Nn, dtype=out_dtype, device=x.q.device)
    _gemm_mxfp8(x, w, y, N.EPI_STORE, bias)
    return y


def linear_resid_mxfp8(x: MxFp8Tensor, w: MxFp8Tensor, bias: Optional[torch.Tensor], resid: Optional[torch.Tensor],
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 ``out = resid + deq(x)·deq(w)ᵀ + bias`` (resid / bias optional; ``out`` may alias ``resid``)."""
    M, Nn, _ = _check_operands(x, w)
    if N.library_path(x.q):
        y = _ref(x, w, bias)
        if resid is not None:
            y = y + resid
        if out is not None:
            out.copy_(y)
            return out
        return y
    if out is None:
        out = torch.empty(M, Nn, dtype=torch.float32, device=x.q.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (M, Nn)
    if resid is not None:
        assert resid.dtype == torch.float32 and resid.is_contiguous() and tuple(resid.shape) == (M, Nn)
        _gemm_mxfp8(x, w, out, N.EPI_RESID, bias, aux=resid)
    else:
        _gemm_mxfp8(x, w, out, N.EPI_STORE, bias)
    return out


def linear_gelu_mxfp8(x: MxFp8Tensor, w: MxFp8Tensor, bias: Optional[torch.Tensor],
                      out_dtype: torch.dtype = torch.bfloat16, quant_out: bool = False):
    """``(d, g)`` for ``u = deq(x)·deq(w)ᵀ + b``: ``d = gelu_tanh'(u)`` and ``g = gelu_tanh(u)``, as
    ``ops.gemm.linear_gelu`` (bf16 on the GPU; ``out_dtype`` applies to the CPU path, whose engine is fp32).
    ``quant_out``: ``(d, g, MxFp8Tensor of g)``, written by the epilogue itself when ``N % 32 == 0`` (and
    ``DTC_MX_FUSE`` is not 0), otherwise by :func:`quant_mxfp8` on ``g``: the same bytes."""
    M, Nn, _ = _check_operands(x, w)
    if quant_out and Nn % BLOCK:
        raise NotImplementedError(f"linear_gelu_mxfp8: the MX form of gelu(u) needs N % 32 == 0, got N={Nn}")
    if N.library_path(x.q):
        u = _ref(x, w, bias)
        d, g = gelu_tanh_grad(u).to(out_dtype), gelu_tanh(u).to(out_dtype)
        return (d, g, quant_mxfp8(g.contiguous())) if quant_out else (d, g)
    if out_dtype != torch.bfloat16:
        raise TypeError(f"linear_gelu_mxfp8: the GPU kernel stores bf16, got {out_dtype}")
    d = torch.empty(M, Nn, dtype=torch.bfloat16, device=x.q.device)
    g = torch.empty_like(d)
    if not quant_out:
        _gemm_mxfp8(x, w, d, N.EPI_GELU, bias, aux_out=g)
        return d, g
    if fuse_enabled():
        gq = empty_like_mx(g)
        _gemm_mxfp8(x, w, d, N.EPI_GELU, bias, aux_out=g, gq=gq)
    else:
        _gemm_mxfp8(x, w, d, N.EPI_GELU, bias, aux_out=g)
        gq = quant_mxfp8(g)
    return d, g, gq
