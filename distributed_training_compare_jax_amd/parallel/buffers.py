"""Flat per-rank parameter / gradient / optimizer-state buffers.

One contiguous fp32 buffer each for master params, grads, Adam m and v (+ a bf16 mirror
of the GEMM-side params) replaces the reference's pytree of 22 leaves.  This is what
makes the MI355X step cheap:

* the fused clip+AdamW (``ops/optim.py``) is ONE launch over the whole buffer;
* DP gradient buckets are plain contiguous slices (grads are laid out in backward
  order), so each RCCL all-reduce / reduce-scatter is one large message;
* wgrad GEMM epilogues write straight into their slice (no autograd accumulation copy);
* checkpoints are a handful of tensors plus an index.

Offsets are 64-element (256-B) aligned for 16-byte vector access.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

from ..models.params import ParamSpec, init_full, local_shape, shard

ALIGN = 64


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


@dataclass
class Slot:
    spec: ParamSpec
    offset: int
    shape: Tuple[int, ...]

    @property
    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n


class FlatParams:
    def __init__(self, specs: List[ParamSpec], tp_rank: int, tp_size: int, device, compute_dtype=torch.bfloat16):
        self.specs = specs
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.device = torch.device(device)
        self.compute_dtype = compute_dtype
        self.slots: Dict[str, Slot] = {}
        off = 0
        n_mirror = 0
        seen_nonmirror = False
        for s in specs:
            shp = local_shape(s, tp_size, tp_rank)
            slot = Slot(s, off, shp)
            self.slots[s.name] = slot
            off = _align(off + slot.numel)
            if s.mirror:
                assert not seen_nonmirror, "mirrored params must precede non-mirrored ones"
                n_mirror = off
            else:
                seen_nonmirror = True
        self.numel = max(off, ALIGN)
        self.n_mirror = n_mirror
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.numel, **f32)
        self.grads = torch.zeros(self.numel, **f32)
        self.exp_avg = torch.zeros(self.numel, **f32)
        self.exp_avg_sq = torch.zeros(self.numel, **f32)
        self.use_mirror = compute_dtype != torch.float32
        self.mirror = (torch.zeros(max(n_mirror, ALIGN), dtype=compute_dtype, device=self.device)
                       if self.use_mirror else None)
        # transposed compute mirror (enable_transposed): name -> (slot, [in, out] bf16 view)
        self.mirror_t: Dict[str, Tuple[Slot, torch.Tensor]] = {}
        self._mirror_t_buf = None
        # FP8 weight mirror (enable_fp8): name -> (slot, ops.fp8.Fp8Tensor), rebuilt wherever the bf16 mirror is
        self.mirror_fp8: Dict[str, Tuple[Slot, object]] = {}
        # MXFP8 weight mirror (enable_mxfp8): name -> (slot, ops.mxfp8.MxFp8Tensor), rebuilt at the same sites
        self.mirror_mx: Dict[str, Tuple[Slot, object]] = {}

    # -- init -----------------------------------------------------------------
    def init_canonical(self, seed: int):
        for name, slot in self.slots.items():
            full = init_full(slot.spec, seed)
            loc = shard(slot.spec, full, self.tp_rank, self.tp_size)
            self.p(name).copy_(loc.to(self.device))
        self.refresh_mirror()

    def refresh_mirror(self):
        if self.use_mirror and self.n_mirror > 0:
            from ..ops.optim import cast_to_bf16

            cast_to_bf16(self.params[: self.n_mirror], self.mirror[: self.n_mirror])
            self.refresh_transposed()
        self.refresh_fp8()
        self.refresh_mxfp8()

    # -- transposed mirror --------------------------------------------------------
    def enable_transposed(self, names: List[str]):
        """Keep a transposed bf16 copy ``[in, out]`` of these 2-D mirrored weights (each rebuilt from
        the mirror after every update: :meth:`refresh_transposed`).  With it a Dense's dgrad
        dX = dY·W runs as an NT GEMM (both operands K-major) on the 8-wave kernels instead of reading
        W k-strided (csrc/gemm.hip; measured in the step, profiles/r2_ab_dgrad_nt.log)."""
        names = [n for n in names if n in self.slots and self.slots[n].spec.mirror and len(self.slots[n].shape) == 2]
        if not names or not self.use_mirror:
            return
        total = sum(self.slots[n].numel for n in names)
        self._mirror_t_buf = torch.zeros(total, dtype=self.compute_dtype, device=self.device)
        off = 0
        for n in names:
            sl = self.slots[n]
            rows, cols = sl.shape
            self.mirror_t[n] = (sl, self._mirror_t_buf[off:off + sl.numel].view(cols, rows))
            off += sl.numel
        self.refresh_transposed()

    def refresh_transposed(self, lo: int = 0, hi: int = None):
        """Rebuild the transposed copies of the weights inside flat[lo:hi] from the bf16 mirror."""
        if not self.mirror_t:
            return
        from ..ops.optim import transpose_batch

        hi = self.numel if hi is None else hi
        transpose_batch([(self._view(self.mirror, n), t) for n, (sl, t) in self.mirror_t.items()
                         if sl.offset >= lo and sl.offset + sl.numel <= hi])

    def transposed_in(self, lo: int, hi: int):
        """[(flat offset, rows, cols, W^T)] of the transposed-mirror weights inside flat[lo:hi]."""
        return [(sl.offset, sl.shape[0], sl.shape[1], t) for sl, t in self.mirror_t.values()
                if sl.offset >= lo and sl.offset + sl.numel <= hi]

    # -- FP8 weight mirror ------------------------------------------------------------
    def enable_fp8(self, names: List[str]):
        """Keep an e4m3 copy (bytes + per-tensor power-of-two scale, ``ops/fp8.py``) of these 2-D mirrored weights:
        ``quant_e4m3`` of the bf16 mirror (of the master rounded to bf16 where no mirror is kept).  Rebuilt by
        :meth:`refresh_fp8` wherever the bf16 mirror is rebuilt or written; not part of a checkpoint."""
        from ..ops import fp8 as F8

        names = [n for n in names if n in self.slots and self.slots[n].spec.mirror and len(self.slots[n].shape) == 2]
        if not names:
            return
        names.sort(key=lambda n: self.slots[n].offset)  # a flat range then holds a run of consecutive entries
        self._fp8_state = F8.new_state(len(names), self.device)
        self._fp8_buf = torch.zeros(sum(self.slots[n].numel for n in names), dtype=torch.uint8, device=self.device)
        off = 0
        for i, n in enumerate(names):
            sl = self.slots[n]
            q = self._fp8_buf[off:off + sl.numel].view(sl.shape)
            self.mirror_fp8[n] = (sl, F8._views(q, self._fp8_state[i]))
            off += sl.numel
        self.refresh_fp8()

    def refresh_fp8(self, lo: int = 0, hi: int = None):
        """Requantise the FP8 copies of the weights inside flat[lo:hi] (one batched quantiser call)."""
        if not self.mirror_fp8:
            return
        from ..ops import fp8 as F8

        hi = self.numel if hi is None else hi
        idx = [i for i, (sl, _) in enumerate(self.mirror_fp8.values()) if sl.offset >= lo and sl.offset + sl.numel <= hi]
        if not idx:
            return
        i0, i1 = idx[0], idx[-1] + 1  # entries are sorted by offset: the ones inside a range are consecutive
        ent = list(self.mirror_fp8.items())[i0:i1]
        src = [self.w(n) if self.use_mirror else self.p(n).to(torch.bfloat16) for n, _ in ent]
        F8.quant_e4m3_batch(src, [t.q for _, (_, t) in ent], self._fp8_state[i0:i1])

    # -- MXFP8 weight mirror -----------------------------------------------------------
    def enable_mxfp8(self, names: List[str]):
        """Keep an MXFP8 copy (e4m3 bytes + one E8M0 scale byte per 32 elements of a row, ``ops/mxfp8.py``) of these
        2-D mirrored weights: ``quant_mxfp8`` of the bf16 mirror (of the master rounded to bf16 where no mirror is
        kept).  Rebuilt by :meth:`refresh_mxfp8` wherever the bf16 mirror is rebuilt or written; not part of a
        checkpoint."""
        from ..ops import mxfp8 as MX

        names = [n for n in names if n in self.slots and self.slots[n].spec.mirror and len(self.slots[n].shape) == 2]
        if not names:
            return
        names.sort(key=lambda n: self.slots[n].offset)
        total = sum(self.slots[n].numel for n in names)
        self._mx_buf = torch.zeros(total, dtype=torch.uint8, device=self.device)
        self._mx_sc = torch.zeros(total // MX.BLOCK, dtype=torch.uint8, device=self.device)
        off = 0
        for n in names:
            sl = self.slots[n]
            rows, cols = sl.shape
            assert cols % MX.BLOCK == 0 and off % MX.BLOCK == 0, (n, sl.shape)
            q = self._mx_buf[off:off + sl.numel].view(rows, cols)
            sc = self._mx_sc[off // MX.BLOCK:(off + sl.numel) // MX.BLOCK].view(rows, cols // MX.BLOCK)
            self.mirror_mx[n] = (sl, MX.MxFp8Tensor(q, sc))
            off += sl.numel
        self.refresh_mxfp8()

    def refresh_mxfp8(self, lo: int = 0, hi: int = None):
        """Requantise the MXFP8 copies of the weights inside flat[lo:hi] (one batched quantiser call)."""
        if not self.mirror_mx:
            return
        from ..ops import mxfp8 as MX

        hi = self.numel if hi is None else hi
        ent = [(n, t) for n, (sl, t) in self.mirror_mx.items() if sl.offset >= lo and sl.offset + sl.numel <= hi]
        if not ent:
            return
        src = [self.w(n) if self.use_mirror else self.p(n).to(torch.bfloat16) for n, _ in ent]
        MX.quant_mxfp8_batch(src, [t for _, t in ent])

    def wmx(self, name: str):
        """The MXFP8 copy of a weight (``ops.mxfp8.MxFp8Tensor``); raises when none is kept."""
        e = self.mirror_mx.get(name)
        if e is None:
            raise KeyError(f"no MXFP8 mirror of {name!r} (FlatParams.enable_mxfp8)")
        return e[1]

    def w8(self, name: str):
        """The e4m3 copy of a weight (``ops.fp8.Fp8Tensor``); raises when none is kept."""
        e = self.mirror_fp8.get(name)
        if e is None:
            raise KeyError(f"no FP8 mirror of {name!r} (FlatParams.enable_fp8)")
        return e[1]

    def wt(self, name: str):
        """Transposed bf16 view ``[in, out]`` of a weight, or None when not kept."""
        e = self.mirror_t.get(name)
        return None if e is None else e[1]

    # -- views ----------------------------------------------------------------
    def _view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        s = self.slots[name]
        return buf[s.offset: s.offset + s.numel].view(s.shape)

    def p(self, name: str) -> torch.Tensor:
        return self._view(self.params, name)

    def g(self, name: str) -> torch.Tensor:
        return self._view(self.grads, name)

    def w(self, name: str) -> torch.Tensor:
        """Compute-dtype view (bf16 mirror on GPU, fp32 master otherwise)."""
        if self.use_mirror and self.slots[name].spec.mirror:
            return self._view(self.mirror, name)
        return self.p(name)

    def has(self, name: str) -> bool:
        return name in self.slots

    def range_of(self, names: List[str]) -> Tuple[int, int]:
        lo = min(self.slots[n].offset for n in names)
        hi = max(_align(self.slots[n].offset + self.slots[n].numel) for n in names)
        return lo, hi

    def segments(self, weight_fn) -> List[Tuple[int, int, float]]:
        return [(s.offset, s.numel, float(weight_fn(s.spec))) for s in self.slots.values()]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"params": self.params, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
