"""Fused clip-by-global-norm + AdamW over flat fp32 buffers.

Reference: ``train/create_optimizer.py:8-12`` —
``optax.chain(clip_by_global_norm(1.0), adamw(lr=3e-4, weight_decay=0.1))`` with optax
defaults (b1 0.9, b2 0.999, eps 1e-8, eps_root 0, bias correction, decoupled decay on
ALL params, no mask):

    g ← g·min(1, max_norm/‖g‖)         (optax: where(‖g‖ < max, g, g/‖g‖·max))
    m ← b1·m + (1−b1)·g ;  v ← b2·v + (1−b2)·g²
    p ← p − lr·( m/(1−b1ᵗ) / (√(v/(1−b2ᵗ)) + eps) + wd·p )

GPU path (``csrc/optim.hip``): (1) a deterministic two-stage Σg² over a segment table
(each segment carries a weight so TP-replicated params are counted once across ranks),
whose finalize kernel also bumps the device step counter; (2) ONE streaming kernel over
the whole flat buffer that applies clip+AdamW and writes the bf16 compute mirror of the
weights — no per-parameter launches, no host sync (graph-capturable).

Parameter groups (``OptimConfig.param_groups``): a :class:`GroupTable` holds the flat buffer as maximal runs of one
(weight decay, rate scale); the same kernels take it (``groups=``) and give every element its run's decay and
``lr (x) scale`` (one fp32 multiply), still in one launch per range.  Without a table the ungrouped entry points
and instantiations run, bit for bit as before.  :func:`last_adamw` records which entry point the last call took.
"""

from __future__ import annotations

import ctypes

from typing import Optional

import torch

from . import _native as N
from .gemm import _workspace


def make_segments(segments, device) -> torch.Tensor:
    """segments: list of (offset, length, weight) → packed float64 tensor [S, 3] for the kernel."""
    t = torch.tensor([[float(o), float(n), float(w)] for (o, n, w) in segments], dtype=torch.float64)
    return t.to(device)


_LAST_ADAMW: dict = {}


def last_adamw() -> dict:
    """Record of the last AdamW call (:func:`adamw_flat` / :func:`adamw_tr`), like ``ops.gemm.last_launch``:
    ``entry`` (the C entry point, or ``cpu``), ``groups`` (whether a group table was applied), ``runs`` (its size),
    ``launches`` (kernel launches of the call), ``n`` / ``base`` of a flat launch."""
    return dict(_LAST_ADAMW)


def _record(entry: str, groups, **kw):
    _LAST_ADAMW.clear()
    _LAST_ADAMW.update(entry=entry, groups=groups is not None, runs=(len(groups.runs) if groups is not None else 0), **kw)


class GroupTable:
    """The flat buffer as maximal runs of one (weight decay, rate scale): ``runs`` = [(lo, hi, wd, lr_scale)] tiling
    [0, numel), every bound a multiple of 64 (slot offsets are 64-aligned; alignment gaps belong to the run before
    them) and neighbouring runs different.  ``ends`` (int64 [R]) and ``hp`` (fp32 [R, 2]) are its device form:
    static memory, built once per ``FlatParams`` before any capture."""

    ALIGN = 64

    def __init__(self, runs, numel: int, device):
        runs = [(int(a), int(b), float(wd), float(s)) for a, b, wd, s in runs]
        assert runs and runs[0][0] == 0 and runs[-1][1] == int(numel), "the runs must tile [0, numel)"
        for i, (a, b, wd, s) in enumerate(runs):
            assert a < b and a % self.ALIGN == 0 and b % self.ALIGN == 0, f"run [{a}, {b}) is not 64-aligned"
            assert i == 0 or runs[i - 1][1] == a, "the runs must be contiguous"
        self.runs, self.numel = runs, int(numel)
        self.ends = torch.tensor([b for _, b, _, _ in runs], dtype=torch.int64).to(device)
        self.hp = torch.tensor([[wd, s] for _, _, wd, s in runs], dtype=torch.float32).reshape(-1, 2).to(device)

    def clip(self, lo: int, hi: int):
        """The runs restricted to [lo, hi): [(a, b, wd, lr_scale)]."""
        return [(max(a, lo), min(b, hi), wd, s) for a, b, wd, s in self.runs if a < hi and b > lo]

    def values_at(self, off: int):
        for a, b, wd, s in self.runs:
            if a <= off < b:
                return a, b, wd, s
        raise IndexError(off)


class LrSchedule:
    """A learning-rate schedule evaluated on the device (``OptimConfig.lr_schedule``: ``warmup_cosine``, ``wsd`` or
    ``warmup_linear``, the last being wsd with a cooldown of N - W: one arithmetic, the same bits).

    ``out`` (fp32 [1]) holds the rate of the current update: the kernel that finishes the global norm and bumps the
    step counter (:func:`sum_finish` / :func:`sumsq_segments` with ``sched=``) writes it, the AdamW kernels read it
    through ``lr_dev=`` instead of their by-value ``lr``.  A captured step therefore replays the schedule, as it
    already replays the bias correction, from the device step counter.  On CPU tensors the same functions write
    ``cfg.lr_at(t)`` rounded to fp32."""

    def __init__(self, cfg, device):
        assert cfg.scheduled
        self.cfg = cfg
        self.lr, self.min_ratio = float(cfg.lr), float(cfg.lr_min_ratio)
        self.warmup, self.decay = int(cfg.lr_warmup_steps), int(cfg.lr_decay_steps)
        # kind 0: warmup_cosine (the entry points and arguments of before); 1: wsd with `cooldown`
        self.kind = 0 if cfg.lr_schedule == "warmup_cosine" else 1
        self.cooldown = int(cfg.cooldown)
        self.out = torch.zeros(1, dtype=torch.float32, device=device)

    @classmethod
    def of(cls, cfg, device) -> "Optional[LrSchedule]":
        return cls(cfg, device) if getattr(cfg, "scheduled", False) else None

    def _write_cpu(self, step: torch.Tensor):
        self.out.fill_(self.cfg.lr_at(int(step[0])))

    def _args(self):
        a = (self.out.data_ptr(), self.lr, self.min_ratio, self.warmup, self.decay)
        return a if self.kind == 0 else a + (self.kind, self.cooldown)

    def _entry(self, base: str) -> str:
        return base + ("_lr" if self.kind == 0 else "_sched")


def _lr_dev(sched: "Optional[LrSchedule]"):
    return None if sched is None else sched.out


def sumsq_segments(flat: torch.Tensor, segments: torch.Tensor, out: torch.Tensor,
                   step: Optional[torch.Tensor] = None, sched: Optional[LrSchedule] = None) -> torch.Tensor:
    """out[0] = Σ_s w_s·Σ_{i∈s} flat[i]²  (fp32).  If ``step`` is given it is incremented by 1, and with ``sched``
    the rate of that update is written to ``sched.out``."""
    assert sched is None or step is not None, "a schedule is evaluated where the step counter is bumped"
    if not flat.is_cuda:
        acc = torch.zeros((), dtype=torch.float64)
        for o, n, w in segments.tolist():
            seg = flat[int(o):int(o) + int(n)].double()
            acc += w * (seg * seg).sum()
        out.fill_(float(acc))
        if step is not None:
            step.add_(1)
        if sched is not None:
            sched._write_cpu(step)
        return out
    L = N.lib()
    ws = _workspace(flat.device, int(L.dtc_sumsq_workspace_bytes()))
    if sched is not None:
        fn = sched._entry("dtc_sumsq_segments")
        N.check(getattr(L, fn)(flat.data_ptr(), segments.data_ptr(), segments.shape[0], out.data_ptr(),
                               N.ptr(step), ws.data_ptr(), ws.numel(), *sched._args(), N.stream_ptr(flat.device)), fn)
        return out
    N.check(L.dtc_sumsq_segments(flat.data_ptr(), segments.data_ptr(), segments.shape[0], out.data_ptr(),
                                 N.ptr(step), ws.data_ptr(), ws.numel(), N.stream_ptr(flat.device)),
            "dtc_sumsq_segments")
    return out


def sumsq_partial(flat: torch.Tensor, segments: torch.Tensor, part: torch.Tensor):
    """part[:] = per-block partial Σ w·g² over ``segments`` (one chunk of an incremental norm)."""
    if not flat.is_cuda:
        acc = torch.zeros((), dtype=torch.float64)
        for o, n, w in segments.tolist():
            seg = flat[int(o):int(o) + int(n)].double()
            acc += w * (seg * seg).sum()
        part.zero_()
        part[0] = float(acc)
        return part
    N.check(N.lib().dtc_sumsq_partial(flat.data_ptr(), segments.data_ptr(), segments.shape[0], part.data_ptr(),
                                      part.numel(), N.stream_ptr(flat.device)), "dtc_sumsq_partial")
    return part


def sum_finish(part: torch.Tensor, out: torch.Tensor, step: Optional[torch.Tensor] = None,
               sched: Optional[LrSchedule] = None) -> torch.Tensor:
    """out[0] = Σ part (fixed order, fp64 accumulate); bumps ``step`` if given (and then, with ``sched``, writes the
    rate of that update to ``sched.out``)."""
    assert sched is None or step is not None, "a schedule is evaluated where the step counter is bumped"
    if not part.is_cuda:
        out.fill_(float(part.double().sum()))
        if step is not None:
            step.add_(1)
        if sched is not None:
            sched._write_cpu(step)
        return out
    if sched is not None:
        fn = sched._entry("dtc_sum_finish")
        N.check(getattr(N.lib(), fn)(part.data_ptr(), part.numel(), out.data_ptr(), N.ptr(step), *sched._args(),
                                     N.stream_ptr(part.device)), fn)
        return out
    N.check(N.lib().dtc_sum_finish(part.data_ptr(), part.numel(), out.data_ptr(), N.ptr(step),
                                   N.stream_ptr(part.device)), "dtc_sum_finish")
    return out


def adamw_flat(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               mirror: Optional[torch.Tensor], n_mirror: int, step: torch.Tensor, sumsq: torch.Tensor,
               lr: float, b1: float, b2: float, eps: float, wd: float, max_norm: float,
               enable: Optional[torch.Tensor] = None, max_blocks: int = 0, lr_dev: Optional[torch.Tensor] = None, *,
               groups: Optional[GroupTable] = None, base: int = 0):
    """In-place AdamW on flat fp32 buffers; ``mirror[:n_mirror] = bf16(p[:n_mirror])``.

    ``groups`` (:class:`GroupTable`, optional) with ``base`` = the flat offset of ``p[0]``: every element takes the
    decay of its run in place of ``wd`` and the rate times its run's scale (one fp32 multiply); the slice may begin
    and end inside runs.  None: the ungrouped kernels.

    ``lr_dev`` (fp32 [1], optional): this update's scheduled rate (:class:`LrSchedule`), read on the device in place
    of ``lr``.

    ``step`` (int64 [1], already incremented) gives t for the bias correction; ``sumsq``
    (fp32 [1]) is the global Σg² for the clip.  ``enable`` (fp32 [1], optional): the update is
    skipped when ``enable[0] == 0`` (device-side switch for the deferred optimizer).  ``max_blocks``
    (GPU, > 0): cap the grid (grid-stride loop) so the pass shares the CUs with concurrent kernels."""
    n = p.numel()
    if groups is not None:
        assert base % 4 == 0 and 0 <= base and base + n <= groups.numel, (base, n, groups.numel)
    if not p.is_cuda:
        if enable is not None and float(enable.item()) == 0.0:
            return
        if groups is not None:  # the same per-run values as the kernel: wd of the run, fp32(lr) * fp32(scale)
            lr32 = lr_dev[0].float().clone() if lr_dev is not None else torch.tensor(lr, dtype=torch.float32)
            for a, b, wd_g, s_g in groups.clip(base, base + n):
                a, b = a - base, b - base
                lr_g = (lr32 * torch.tensor(s_g, dtype=torch.float32)).reshape(1)
                k = min(max(n_mirror - a, 0), b - a)
                adamw_flat(p[a:b], g[a:b], m[a:b], v[a:b], mirror[a:] if (mirror is not None and k > 0) else None, k,
                           step, sumsq, 0.0, b1, b2, eps, wd_g, max_norm, lr_dev=lr_g)
            _record("cpu", groups, launches=0, n=n, base=base)
            return
        _record("cpu", None, launches=0, n=n, base=base)
        # the hyperparameters as the kernel gets them: fp32 roundings, 1 - b formed in fp32 (1 - 0.999 in double
        # rounds to an fp32 1.3e-5 away from 1.f - 0.999f)
        lr, b1, b2, eps, wd, mx = (torch.tensor(x, dtype=torch.float32) for x in (lr, b1, b2, eps, wd, max_norm))
        if lr_dev is not None:
            lr = lr_dev[0].float().clone()
        t = step[0].float()
        norm = sumsq[0].float().sqrt()
        scale = mx / norm if (max_norm > 0 and not bool(norm < mx)) else torch.tensor(1.0)
        gg = g * scale
        m.mul_(b1).add_((1 - b1) * gg)
        v.mul_(b2).add_(((1 - b2) * gg) * gg)
        mhat = m / (1 - torch.pow(b1, t))
        vhat = v / (1 - torch.pow(b2, t))
        p.sub_(lr * (mhat / (vhat.sqrt() + eps) + wd * p))
        if mirror is not None and n_mirror > 0:
            mirror[:n_mirror].copy_(p[:n_mirror])
        return
    if groups is not None:
        assert groups.ends.device == p.device
        N.check(N.lib().dtc_adamw_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(mirror), n,
                                         n_mirror, step.data_ptr(), sumsq.data_ptr(), lr, b1, b2, eps, wd, max_norm,
                                         N.ptr(enable), int(max_blocks), N.ptr(lr_dev), groups.ends.data_ptr(),
                                         groups.hp.data_ptr(), len(groups.runs), int(base), groups.numel,
                                         N.stream_ptr(p.device)), "dtc_adamw_groups")
        _record("dtc_adamw_groups", groups, launches=1, n=n, base=base)
        return
    _record("dtc_adamw_lr" if lr_dev is not None else "dtc_adamw", None, launches=1, n=n, base=base)
    if lr_dev is not None:
        N.check(N.lib().dtc_adamw_lr(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(mirror), n, n_mirror,
                                     step.data_ptr(), sumsq.data_ptr(), lr, b1, b2, eps, wd, max_norm, N.ptr(enable),
                                     int(max_blocks), lr_dev.data_ptr(), N.stream_ptr(p.device)), "dtc_adamw_lr")
        return
    N.check(N.lib().dtc_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(mirror), n, n_mirror,
                              step.data_ptr(), sumsq.data_ptr(), lr, b1, b2, eps, wd, max_norm, N.ptr(enable),
                              int(max_blocks), N.stream_ptr(p.device)), "dtc_adamw")


def cast_to_bf16(src: torch.Tensor, dst: torch.Tensor):
    if not src.is_cuda:
        dst.copy_(src)
        return
    N.check(N.lib().dtc_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), N.stream_ptr(src.device)),
            "dtc_cast_f32_bf16")


class _TrTask(ctypes.Structure):
    """Mirror of ``struct TrTask`` (csrc/elementwise.hip)."""

    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("blk0", ctypes.c_int), ("pad", ctypes.c_int)]


_TR_MAX = 32


class _TrBatch(ctypes.Structure):
    _fields_ = [("ntasks", ctypes.c_int), ("nblocks", ctypes.c_int), ("t", _TrTask * _TR_MAX)]


def transpose_batch(pairs):
    """dst = src.T for each (src [rows, cols], dst [cols, rows]) bf16 pair: one launch per 32 matrices
    on GPU (the transposed weight mirror), torch on CPU."""
    if not pairs:
        return
    if not pairs[0][0].is_cuda:
        for src, dst in pairs:
            dst.copy_(src.t())
        return
    L = N.lib()
    assert L.dtc_tr_task_bytes() == ctypes.sizeof(_TrTask) and L.dtc_tr_max_tasks() == _TR_MAX
    for i in range(0, len(pairs), _TR_MAX):
        chunk = pairs[i:i + _TR_MAX]
        b = _TrBatch()
        b.ntasks = len(chunk)
        blk = 0
        for j, (src, dst) in enumerate(chunk):
            rows, cols = src.shape
            assert tuple(dst.shape) == (cols, rows) and src.is_contiguous() and dst.is_contiguous()
            b.t[j] = _TrTask(src.data_ptr(), dst.data_ptr(), rows, cols, blk, 0)
            blk += ((rows + 63) // 64) * ((cols + 63) // 64)
        b.nblocks = blk
        N.check(L.dtc_transpose_batch(ctypes.byref(b), N.stream_ptr(src.device)), "dtc_transpose_batch")


class _AwSeg(ctypes.Structure):
    """Mirror of ``struct AwSeg`` (csrc/elementwise.hip)."""

    _fields_ = [("lo", ctypes.c_long), ("n", ctypes.c_long), ("blk0", ctypes.c_int), ("pad", ctypes.c_int),
                ("wd", ctypes.c_float), ("lr_scale", ctypes.c_float)]


_AW_SEG_MAX, _AW_TASK_MAX = 96, 64


class _AwSegs(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int), ("nblocks", ctypes.c_int), ("s", _AwSeg * _AW_SEG_MAX)]


class _AwtTask(ctypes.Structure):
    _fields_ = [("off", ctypes.c_long), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("blk0", ctypes.c_int), ("pad", ctypes.c_int), ("wd", ctypes.c_float), ("lr_scale", ctypes.c_float)]


class _AwtBatch(ctypes.Structure):
    _fields_ = [("ntasks", ctypes.c_int), ("nblocks", ctypes.c_int), ("t", _AwtTask * _AW_TASK_MAX)]


class _GroupedPlan(list):
    """An :func:`adamw_tr_plan` whose segments and tiles carry their run's (wd, lr_scale): the grouped kernels."""

    grouped = True
    runs = 0


def adamw_tr_plan(lo: int, hi: int, mats, *, groups: Optional[GroupTable] = None):
    """Launch lists of :func:`adamw_tr` over flat[lo:hi]: ``mats`` = [(offset, rows, cols, W^T tensor)] of the
    weights that keep a transposed mirror (inside the range).  Returns [(segments, tiles)] chunks (each
    within the kernels' list capacities), or None when a shape does not fit the tiled kernel.

    ``groups``: the segments are split at the table's run bounds and every segment and tile carries its run's
    (wd, lr_scale) (a weight is one parameter, hence inside one run); the lists stay kernel arguments (32 B x 96
    segments = 3.1 KB, 40 B x 64 tiles = 2.6 KB, under the 4 KB of a launch) and a plan with more entries than one
    list holds goes out in several launches, as before."""
    mats = sorted(mats, key=lambda x: x[0])
    if any(r % 8 or c % 4 or o % 4 for o, r, c, _ in mats):
        return None
    segs, cur = [], lo
    for o, r, c, _ in mats:
        if o > cur:
            segs.append((cur, o - cur))
        cur = o + r * c
    if hi > cur:
        segs.append((cur, hi - cur))
    if any(a % 4 or n % 4 for a, n in segs):
        return None
    hp_of = {}
    if groups is not None:
        assert 0 <= lo and hi <= groups.numel
        split = []
        for a, n in segs:
            for ra, rb, wd_g, s_g in groups.clip(a, a + n):
                split.append((ra, rb - ra))
                hp_of[ra] = (wd_g, s_g)
        segs = split
        for o, r, c, _ in mats:
            ra, rb, wd_g, s_g = groups.values_at(o)
            assert o + r * c <= rb, f"the weight at {o} ({r} x {c}) straddles a run bound of the group table"
            hp_of[o] = (wd_g, s_g)
    chunks = []
    while segs or mats:
        sb, tb = _AwSegs(), _AwtBatch()
        blk = 0
        take = segs[:_AW_SEG_MAX]
        segs = segs[_AW_SEG_MAX:]
        for j, (a, n) in enumerate(take):
            sb.s[j] = _AwSeg(a, n, blk, 0, *hp_of.get(a, (0.0, 0.0)))
            blk += (n + 4095) // 4096
        sb.nseg, sb.nblocks = len(take), blk
        blk = 0
        tk = mats[:_AW_TASK_MAX]
        mats = mats[_AW_TASK_MAX:]
        for j, (o, r, c, dst) in enumerate(tk):
            assert tuple(dst.shape) == (c, r) and dst.is_contiguous()
            tb.t[j] = _AwtTask(o, dst.data_ptr(), r, c, blk, 0, *hp_of.get(o, (0.0, 0.0)))
            blk += ((r + 63) // 64) * ((c + 63) // 64)
        tb.ntasks, tb.nblocks = len(tk), blk
        chunks.append((sb, tb))
    if groups is not None:
        chunks = _GroupedPlan(chunks)
        chunks.runs = len(groups.runs)
    return chunks


def adamw_tr(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, mirror: torch.Tensor, n_mirror: int,
             plan, step: torch.Tensor, sumsq: torch.Tensor, lr: float, b1: float, b2: float, eps: float, wd: float,
             max_norm: float, lr_dev: Optional[torch.Tensor] = None):
    """AdamW over the flat buffers (absolute offsets in ``plan``, :func:`adamw_tr_plan`) with the transposed
    bf16 mirror of the tiled weights written by the update itself (no separate transpose pass).  GPU only;
    bitwise equal to :func:`adamw_flat` + :func:`transpose_batch`.  A plan built with ``groups=`` runs the grouped
    kernels (each segment / tile with its own decay and rate scale)."""
    L = N.lib()
    assert L.dtc_aw_seg_bytes() == ctypes.sizeof(_AwSeg) and L.dtc_aw_task_bytes() == ctypes.sizeof(_AwtTask)
    assert L.dtc_aw_max_seg() == _AW_SEG_MAX and L.dtc_aw_max_tasks() == _AW_TASK_MAX
    assert ctypes.sizeof(_AwSegs) < 4096 and ctypes.sizeof(_AwtBatch) < 4096  # kernel arguments
    grouped = bool(getattr(plan, "grouped", False))
    launches = sum((sb.nseg > 0 and sb.nblocks > 0) + (tb.ntasks > 0 and tb.nblocks > 0) for sb, tb in plan)
    _LAST_ADAMW.clear()
    _LAST_ADAMW.update(entry="dtc_adamw_tr_groups" if grouped else ("dtc_adamw_tr_lr" if lr_dev is not None
                                                                     else "dtc_adamw_tr"),
                       groups=grouped, runs=getattr(plan, "runs", 0), launches=int(launches), chunks=len(plan))
    for sb, tb in plan:
        if grouped:
            N.check(L.dtc_adamw_tr_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror.data_ptr(),
                                          n_mirror, ctypes.byref(sb), ctypes.byref(tb), step.data_ptr(),
                                          sumsq.data_ptr(), lr, b1, b2, eps, wd, max_norm, N.ptr(lr_dev),
                                          N.stream_ptr(p.device)), "dtc_adamw_tr_groups")
            continue
        if lr_dev is not None:
            N.check(L.dtc_adamw_tr_lr(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror.data_ptr(),
                                      n_mirror, ctypes.byref(sb), ctypes.byref(tb), step.data_ptr(), sumsq.data_ptr(),
                                      lr, b1, b2, eps, wd, max_norm, lr_dev.data_ptr(), N.stream_ptr(p.device)),
                    "dtc_adamw_tr_lr")
            continue
        N.check(L.dtc_adamw_tr(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), mirror.data_ptr(), n_mirror,
                               ctypes.byref(sb), ctypes.byref(tb), step.data_ptr(), sumsq.data_ptr(), lr, b1, b2, eps,
                               wd, max_norm, N.stream_ptr(p.device)), "dtc_adamw_tr")


def fill_(t: torch.Tensor, value: float):
    """t[:] = value (fp32; graph-capturable on GPU)."""
    if not t.is_cuda:
        t.fill_(value)
        return t
    N.check(N.lib().dtc_fill_f32(t.data_ptr(), value, t.numel(), N.stream_ptr(t.device)), "dtc_fill_f32")
    return t
