"""FP8 (OCP ``e4m3fn``) forward path: the per-tensor power-of-two quantiser and the layer GEMMs on it.

Quantiser (the torch CPU path below is the definition; ``csrc/gemm_fp8.hip`` agrees with it bit for bit):

* ``amax = max|x|`` exactly;
* with ``e = floor(log2(amax))`` the scale is ``s = 2^(8-e)``, or ``2^(7-e)`` when ``amax·s > 448``, so that
  ``amax·s`` lies in (224, 448]; ``amax == 0`` gives ``s = 1``; the exponent of ``s`` is clamped to [-126, 126] so
  that ``s`` and ``1/s`` are normal fp32;
* ``q = RNE_e4m3(x·s)``: ``x·s`` is exact in fp32, so one rounding, and never above 448.  Inputs are finite.

amax, ``s`` and ``1/s`` live on the device (no ``.item()``): the GEMM reads ``1/s`` through device pointers, so a
step that quantises still captures and replays as a hipGraph.

GEMMs (NT only: ``C = (Aq·Bqᵀ)/(sa·sb)`` + epilogue, ``K % 128 == 0``, ``N % 16 == 0``, any ``M >= 1``; anything
else raises ``NotImplementedError`` before a launch): :func:`linear_fp8`, :func:`linear_resid_fp8`,
:func:`linear_gelu_fp8`, the FP8 forms of ``ops.gemm.linear`` / ``linear_resid`` / ``linear_gelu``.  CPU tensors
compute on the dequantised operands in fp32.
"""

from __future__ import annotations

import collections
import ctypes
from typing import List, Optional, Sequence

import torch

from . import _native as N
from .gemm import gelu_tanh, gelu_tanh_grad

E4M3_MAX = 448.0

# q: uint8 [M, K] (e4m3fn bytes); scale, inv: fp32 [1] device tensors (s and 1/s)
Fp8Tensor = collections.namedtuple("Fp8Tensor", "q scale inv")


class QuantTask(ctypes.Structure):
    """Mirror of ``struct QuantTask`` in csrc/gemm_fp8.hip (keep in sync)."""

    _fields_ = [("src", N.c_vp), ("q", N.c_vp), ("st", N.c_vp), ("n", N.c_long), ("blk0", N.c_int),
                ("nblk", N.c_int), ("f32", N.c_int), ("pad", N.c_int)]


QT_MAX = 64  # csrc/gemm_fp8.hip QT_MAX


class QuantBatch(ctypes.Structure):
    _fields_ = [("ntasks", N.c_int), ("nblocks", N.c_int), ("t", QuantTask * QT_MAX)]


class Fp8GemmArgs(ctypes.Structure):
    """Mirror of ``struct Fp8GemmArgs`` in csrc/gemm_fp8.hip (keep in sync)."""

    _fields_ = [
        ("M", N.c_int), ("N", N.c_int), ("K", N.c_int),
        ("A", N.c_vp), ("lda", N.c_long),
        ("B", N.c_vp), ("ldb", N.c_long),
        ("C", N.c_vp), ("ldc", N.c_long),
        ("c_f32", N.c_int), ("epi", N.c_int),
        ("bias", N.c_vp),
        ("aux", N.c_vp), ("ldaux", N.c_long),
        ("aux_out", N.c_vp),
        ("inv_sa", N.c_vp), ("inv_sb", N.c_vp),
    ]


# ----------------------------------------------------------------------------- quantiser
def scale_from_amax(amax: torch.Tensor):
    """``(s, 1/s)`` for an fp32 ``amax`` tensor (any shape), by the rule in the module docstring."""
    amax = amax.float()
    m, ex = torch.frexp(amax)  # amax = m·2^ex with m in [0.5, 1): e = ex - 1, and amax·2^(8-e) > 448 <=> m > 0.875
    se = torch.where(m > 0.875, 8 - ex, 9 - ex).clamp(-126, 126)
    one = torch.ones_like(amax)
    pos = amax > 0
    return torch.where(pos, torch.ldexp(one, se), one), torch.where(pos, torch.ldexp(one, -se), one)


def _quant_cpu(x: torch.Tensor) -> Fp8Tensor:
    xf = x.float()
    s, inv = scale_from_amax(xf.abs().max().reshape(1))
    q = (xf * s).to(torch.float8_e4m3fn).view(torch.uint8)
    return Fp8Tensor(q, s, inv)


def dequant(t: Fp8Tensor) -> torch.Tensor:
    """fp32 values of a quantised tensor: ``e4m3(q) / s`` (exact)."""
    return t.q.view(torch.float8_e4m3fn).float() * t.inv.to(t.q.device)


_QT_CHECKED = [False]
_BLOCK_ELEMS = 8192  # 256 threads x 4 vectors of 8 elements per block
_MAX_BLOCKS = 512    # per tensor; the kernels stride


def new_state(n: int, device) -> torch.Tensor:
    """The per-tensor quantiser state of ``n`` tensors: int32 ``[n, 4]`` = (amax bits, s, 1/s, pad)."""
    return torch.zeros(n, 4, dtype=torch.int32, device=device)


def _views(q: torch.Tensor, st_row: torch.Tensor) -> Fp8Tensor:
    f = st_row.view(torch.float32)
    return Fp8Tensor(q, f[1:2], f[2:3])


def quant_e4m3_batch(xs: Sequence[torch.Tensor], qs: Optional[Sequence[torch.Tensor]] = None,
                     st: Optional[torch.Tensor] = None) -> List[Fp8Tensor]:
    """Quantise a list of tensors: per chunk of :data:`QT_MAX` tensors one amax launch plus one quantise launch
    over a task table.  ``qs`` / ``st`` (:func:`new_state`): preallocated outputs (a persistent mirror)."""
    xs = list(xs)
    if not xs:
        return []
    for x in xs:
        if x.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"quant_e4m3: bf16 or fp32 input, got {x.dtype}")
        if not x.is_contiguous() or x.numel() == 0:
            raise ValueError(f"quant_e4m3: expected a non-empty contiguous tensor, got shape {tuple(x.shape)} "
                             f"strides {x.stride()}")
    if N.library_path(xs[0]):
        out = [_quant_cpu(x) for x in xs]
        if qs is not None:
            for o, q in zip(out, qs):
                q.copy_(o.q)
            for i, o in enumerate(out):
                f = st[i].view(torch.float32)
                f[1], f[2] = o.scale[0], o.inv[0]
                st[i, 0] = xs[i].float().abs().max().view(torch.int32)
            out = [_views(q, st[i]) for i, q in enumerate(qs)]
        return out
    dev = xs[0].device
    if qs is None:
        qs = [torch.empty(x.shape, dtype=torch.uint8, device=dev) for x in xs]
    if st is None:
        st = torch.empty(len(xs), 4, dtype=torch.int32, device=dev)
    assert st.dtype == torch.int32 and tuple(st.shape) == (len(xs), 4) and st.is_contiguous() and st.device == dev
    L = N.lib()
    if not _QT_CHECKED[0]:
        assert L.dtc_qt_max() == QT_MAX and L.dtc_qt_task_bytes() == ctypes.sizeof(QuantTask)
        assert L.dtc_qt_batch_bytes() == ctypes.sizeof(QuantBatch)
        _QT_CHECKED[0] = True
    for i0 in range(0, len(xs), QT_MAX):
        b = QuantBatch()
        blk = 0
        chunk = range(i0, min(i0 + QT_MAX, len(xs)))
        for j, i in enumerate(chunk):
            x, q = xs[i], qs[i]
            assert q.dtype == torch.uint8 and q.is_contiguous() and q.numel() == x.numel() and q.device == dev
            if x.data_ptr() % 16 or q.data_ptr() % 8:
                raise ValueError("quant_e4m3: the input must be 16-byte aligned and the output 8-byte aligned")
            nblk = max(1, min(_MAX_BLOCKS, (x.numel() + _BLOCK_ELEMS - 1) // _BLOCK_ELEMS))
            b.t[j] = QuantTask(x.data_ptr(), q.data_ptr(), st[i].data_ptr(), x.numel(), blk, nblk,
                               1 if x.dtype == torch.float32 else 0, 0)
            blk += nblk
        b.ntasks, b.nblocks = len(chunk), blk
        N.check(L.dtc_quant_e4m3_tasks(ctypes.byref(b), st[i0].data_ptr(), 16 * len(chunk), N.stream_ptr(dev)),
                "dtc_quant_e4m3_tasks")
    return [_views(q, st[i]) for i, q in enumerate(qs)]


def quant_e4m3(x: torch.Tensor) -> Fp8Tensor:
    """``(q, scale, inv)`` of a bf16 or fp32 row-major ``[M, K]`` tensor (see the module docstring)."""
    if x.dim() != 2:
        raise ValueError(f"quant_e4m3: expected a 2-D tensor, got shape {tuple(x.shape)}")
    return quant_e4m3_batch([x])[0]


# ----------------------------------------------------------------------------- GEMM
VARIANTS = {4: "fp8_128x128", 2: "fp8_64x128"}
EPI_NAMES = {N.EPI_STORE: "bias", N.EPI_RESID: "bias_resid", N.EPI_GELU: "gelu_pair"}

LastLaunchFp8 = collections.namedtuple("LastLaunchFp8", "tile variant epilogue out_f32 blocks")


def last_launch_fp8() -> LastLaunchFp8:
    """What the last FP8 GEMM launch of this process ran, as recorded by the launch site (csrc/gemm_fp8.hip
    ``launch_fp8``, from the kernel's own template arguments): the ``tile`` (rows, columns), the ``variant`` (one of
    :data:`VARIANTS`), the ``epilogue`` (one of :data:`EPI_NAMES`), whether the store was fp32 and the grid size.
    Tests assert it; nothing on the hot path reads it."""
    out = (ctypes.c_int * 8)()
    N.check(N.lib().dtc_gemm_fp8_last_launch(out), "dtc_gemm_fp8_last_launch")
    v = list(out)
    variant = VARIANTS.get(v[2], "none")
    if v[6]:  # the launch was an MX kernel of the same tile (ops/mxfp8.py last_launch_mxfp8 says more)
        variant = "mx" + variant
    return LastLaunchFp8((v[0], v[1]), variant, EPI_NAMES.get(v[3], "none"), bool(v[4]), v[5])


def set_tile_m(bm: int = 0):
    """A/B switch of the tile height: 0 = chosen by grid size (the default), 64 or 128 = forced."""
    N.check(N.lib().dtc_gemm_fp8_set_tile_m(int(bm)), "dtc_gemm_fp8_set_tile_m")


def _check_operands(x: Fp8Tensor, w: Fp8Tensor):
    for t, name in ((x, "x"), (w, "w")):
        if t.q.dim() != 2 or t.q.dtype != torch.uint8 or t.q.stride(1) != 1:
            raise ValueError(f"{name}: expected row-major 2-D e4m3 bytes (uint8), got {t.q.dtype} shape "
                             f"{tuple(t.q.shape)} strides {t.q.stride()}")
    M, K = x.q.shape
    Nn, Kw = w.q.shape
    if Kw != K:
        raise ValueError(f"linear_fp8: x is [{M}, {K}] but w is [{Nn}, {Kw}]")
    if M < 1 or K % 128 or K < 128 or Nn % 16 or Nn < 16:
        raise NotImplementedError(f"FP8 GEMM needs M >= 1, K % 128 == 0 and N % 16 == 0, got M={M} N={Nn} K={K}")
    return M, Nn, K


def _gemm_fp8(x: Fp8Tensor, w: Fp8Tensor, c: torch.Tensor, epi: int, bias, aux=None, aux_out=None):
    M, K = x.q.shape
    Nn = w.q.shape[0]
    if x.q.stride(0) % 16 or w.q.stride(0) % 16 or x.q.data_ptr() % 16 or w.q.data_ptr() % 16:
        raise ValueError("FP8 GEMM operands must be 16-byte aligned with row strides that are multiples of 16")
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Nn
    args = Fp8GemmArgs(M=M, N=Nn, K=K, A=x.q.data_ptr(), lda=x.q.stride(0), B=w.q.data_ptr(), ldb=w.q.stride(0),
                       C=c.data_ptr(), ldc=Nn, c_f32=1 if c.dtype == torch.float32 else 0, epi=epi, bias=N.ptr(bias),
                       aux=N.ptr(aux), ldaux=Nn, aux_out=N.ptr(aux_out), inv_sa=x.inv.data_ptr(),
                       inv_sb=w.inv.data_ptr())
    N.check(N.lib().dtc_gemm_fp8(ctypes.byref(args), N.stream_ptr(c.device)), "dtc_gemm_fp8")


def _ref(x: Fp8Tensor, w: Fp8Tensor, bias):
    y = dequant(x) @ dequant(w).t()
    return y if bias is None else y + bias.float()


def linear_fp8(x: Fp8Tensor, w: Fp8Tensor, bias: Optional[torch.Tensor] = None,
               out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``y = deq(x)·deq(w)ᵀ + b`` (bf16 or fp32 out)."""
    M, Nn, _ = _check_operands(x, w)
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"linear_fp8: bf16 or fp32 output, got {out_dtype}")
    if N.library_path(x.q):
        return _ref(x, w, bias).to(out_dtype)
    y = torch.empty(M, Nn, dtype=out_dtype, device=x.q.device)
    _gemm_fp8(x, w, y, N.EPI_STORE, bias)
    return y


def linear_resid_fp8(x: Fp8Tensor, w: Fp8Tensor, bias: Optional[torch.Tensor], resid: Optional[torch.Tensor],
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
        _gemm_fp8(x, w, out, N.EPI_RESID, bias, aux=resid)
    else:
        _gemm_fp8(x, w, out, N.EPI_STORE, bias)
    return out


def linear_gelu_fp8(x: Fp8Tensor, w: Fp8Tensor, bias: Optional[torch.Tensor],
                    out_dtype: torch.dtype = torch.bfloat16):
    """``(d, g)`` for ``u = deq(x)·deq(w)ᵀ + b``: ``d = gelu_tanh'(u)`` and ``g = gelu_tanh(u)``, as
    ``ops.gemm.linear_gelu`` (bf16 on the GPU; ``out_dtype`` applies to the CPU path, whose engine is fp32)."""
    M, Nn, _ = _check_operands(x, w)
    if N.library_path(x.q):
        u = _ref(x, w, bias)
        return gelu_tanh_grad(u).to(out_dtype), gelu_tanh(u).to(out_dtype)
    if out_dtype != torch.bfloat16:
        raise TypeError(f"linear_gelu_fp8: the GPU kernel stores bf16, got {out_dtype}")
    d = torch.empty(M, Nn, dtype=torch.bfloat16, device=x.q.device)
    g = torch.empty_like(d)
    _gemm_fp8(x, w, d, N.EPI_GELU, bias, aux_out=g)
    return d, g
