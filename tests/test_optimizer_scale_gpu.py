"""The optimizer step, element by element, against float64 optax semantics (docs/NUMERICS.md, "Optimizer").

``test_kernels_gpu.py::test_adamw_matches_cpu`` applies one gradient three times from ``m = v = 0``: the update is
``+-lr`` on every element whatever ``b1`` is, however ``m`` is stored and wherever the weight decay sits, ``m`` is
never compared, and the reference is the CPU branch of the function under test.  Here states and gradients span
decades, the reference is a float64 function written from the optax chain that uses nothing from ``ops/``, and
``m``, ``v`` and ``p`` are bounded per element by ``T * 2^-24 * (sum of the absolute terms)`` with
``T = 4 x the floor of an fp32 torch evaluation of the same case on the same data``.  The only absolute term is
``2^-126`` (nothing is asserted about denormal flushing).  The norm kernels are held to a relative bound derived
from their accumulation depth on data whose every edge element carries a visible share of the sum.

The ``test_selfcheck_*`` tests and the ``cpu`` parametrisation of the end-to-end test need no GPU.
"""

import functools
import math

import pytest
import torch

from test_kernels_gpu import _close, _r

from distributed_training_compare_jax_amd.ops import optim as O

gpu = pytest.mark.gpu

U24 = 2.0 ** -24      # unit roundoff of fp32
TINY = 2.0 ** -126    # smallest normal fp32: the only absolute term of any bound
MARGIN = 4.0          # device powf / sqrtf / division at 1-2 ulp where the CPU's are correctly rounded, fmaf grouping
POW_ULPS = 2.0        # error allowed to fp32 powf in the bias corrections (kappa)
GUARD = 64            # sentinel elements before and after every buffer
SENT_BF16 = 7.0       # sentinel of the bf16 buffers (mirror, W^T)
NAN = float("nan")

# (lr, b1, b2, eps, wd)
HP = ((3e-4, 0.9, 0.999, 1e-8, 0.1), (3e-4, 0.9, 0.95, 1e-5, 0.0))
STEPS = (1, 2, 7, 1000, 100000)
# name -> (the fp32 sum of squares handed to the kernel, max_norm): the kernel takes the norm as an input, so the
# test picks the clip through it
CLIPS = {"inactive": (0.25, 1.0), "exact": (1.0, 1.0), "active": (1e6, 1.0), "off": (1e6, 0.0),
         "inf": (float("inf"), 1.0), "nan": (NAN, 1.0)}
N_MAIN = 65540


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# -------------------------------------------------------------------------------------------------- data

@functools.lru_cache(maxsize=None)
def _data(n, seed=0):
    """(p0, g, m0, v0) fp32 on the CPU, shared by every case and never modified.  |g| log-uniform over
    1e-12 .. 1e2, |p| over 1e-6 .. 10, m0 = 0.5 randn |g| (b1 m0 and (1-b1) g cancel in part), v0 = g^2 10^U(-1,1).
    By index modulo 16, so that every prefix holds the same proportions: 0 -> m0 = v0 = 0 and |g| <= 1e-9 (the
    eps regime), 1 -> g = 0 exactly (pure decay of m, v, p), 2 -> |g| ~ 1e-22 (g^2 underflows in fp32)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    rand = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sign = lambda: torch.where(rand() < 0.5, -1.0, 1.0).double()
    regime = torch.arange(n) % 16
    absg = 10 ** (rand() * 14 - 12)
    absg = torch.where(regime == 0, 10 ** (rand() * 3 - 12), absg)
    absg = torch.where(regime == 2, 1e-22 * (1 + rand()), absg)
    g = absg * sign()
    p = 10 ** (rand() * 7 - 6) * sign()
    m0 = 0.5 * torch.randn(n, generator=gen, dtype=torch.float64) * absg
    v0 = absg * absg * 10 ** (rand() * 2 - 1)
    m0 = torch.where(regime == 0, 0.0, m0)
    v0 = torch.where(regime == 0, 0.0, v0)
    g = torch.where(regime == 1, 0.0, g)
    return tuple(t.float() for t in (p, g, m0, v0))


# --------------------------------------------------------------------------------------------- reference

def _kappa(t, b1, b2, share=1.0):
    """fp32 powf in the bias corrections: POW_ULPS ulp of b^t is a relative error POW_ULPS 2^-24 b^t / (1 - b^t)
    of 1 - b^t.  m-hat takes that of b1 in full; sqrt(v-hat) takes half of that of b2, and u = m-hat / (sqrt(v-hat)
    + eps) the ``share`` = sqrt(v-hat) / (sqrt(v-hat) + eps) of it (1 where eps does not matter, 0 where it is all
    of the denominator).  In units of 2^-24 |u|."""
    f = lambda b: b ** t / (1.0 - b ** t)
    return POW_ULPS * (f(_f32(b1)) + 0.5 * f(_f32(b2)) * share)


def _ref64(data, t, sumsq, hp, max_norm, kappa=None):
    """clip_by_global_norm + adamw in float64, from the optax chain: hyperparameters as their fp32 roundings (the
    C ABI passes floats), ``sumsq`` the fp32 value the kernel is given.  ``max_norm = 0`` is this project's "no
    clip".  Returns the new (p, m, v) and the per-element bounds at T = 1, without the 2^-126."""
    lr, b1, b2, eps, wd = (_f32(x) for x in hp)
    p0, g, m0, v0 = (x.double() for x in data)
    norm = torch.tensor(sumsq, dtype=torch.float32).double().sqrt()
    gc = torch.where(norm < max_norm, g, g / norm * max_norm) if max_norm > 0 else g
    m = b1 * m0 + (1 - b1) * gc
    v = b2 * v0 + (1 - b2) * gc * gc
    rv = (v / (1 - b2 ** t)).sqrt()
    u = (m / (1 - b1 ** t)) / (rv + eps)
    p = p0 - lr * (u + wd * p0)
    k = _kappa(t, b1, b2, rv / (rv + eps)) if kappa is None else kappa
    unit = {"m": U24 * ((b1 * m0).abs() + ((1 - b1) * gc).abs()),
            "v": U24 * v,
            "p": U24 * (p.abs() + lr * (u.abs() * (1 + k) + wd * p0.abs()))}
    return {"p": p, "m": m, "v": v}, unit


MUTANTS = ("b1 = 0.8", "m stored through bf16", "decay on the updated p", "m from the unclipped gradient",
           "bias correction at t-1", "eps under the root", "eps dropped", "v stored through bf16")


def _emulate32(data, t, sumsq, hp, max_norm, mutant=None):
    """The same formula in fp32 torch on the CPU (fp32 ``torch.pow``, no kernel involved): its error against
    ``_ref64`` is the floor an fp32 implementation sits on.  ``mutant``: one of MUTANTS, for the self-checks."""
    assert mutant is None or mutant in MUTANTS
    p0, g, m0, v0 = data
    lr, b1, b2, eps, wd = (torch.tensor(x, dtype=torch.float32) for x in hp)
    if mutant == "b1 = 0.8":
        b1 = torch.tensor(0.8, dtype=torch.float32)
    norm = torch.tensor(sumsq, dtype=torch.float32).sqrt()
    mx = torch.tensor(max_norm, dtype=torch.float32)
    c = mx / norm if (max_norm > 0 and not bool(norm < mx)) else torch.tensor(1.0)
    gc = g * c
    m = b1 * m0 + (1 - b1) * (g if mutant == "m from the unclipped gradient" else gc)
    v = b2 * v0 + ((1 - b2) * gc) * gc
    if mutant == "m stored through bf16":
        m = m.to(torch.bfloat16).float()
    if mutant == "v stored through bf16":
        v = v.to(torch.bfloat16).float()
    tt = torch.tensor(float(t - 1 if mutant == "bias correction at t-1" else t), dtype=torch.float32)
    mh, vh = m / (1 - torch.pow(b1, tt)), v / (1 - torch.pow(b2, tt))
    if mutant == "eps under the root":
        den = (vh + eps).sqrt()
    elif mutant == "eps dropped":
        den = vh.sqrt()
    else:
        den = vh.sqrt() + eps
    if mutant == "decay on the updated p":
        p = p0 - lr * (mh / den)
        p = p - (lr * wd) * p
    else:
        p = p0 - lr * (mh / den + wd * p0)
    return {"p": p, "m": m, "v": v}


def _ratios(out, ref, unit, n=None):
    """max over the elements of (|out - ref| - 2^-126)+ / unit per tensor: the T the result would need.  An error
    where the unit is 0 counts as inf, a NaN as inf.  ``n``: the outputs cover the first n elements only."""
    res = {}
    for k in ("m", "v", "p"):
        o = out[k].detach().cpu().double()
        r, un = (ref[k], unit[k]) if n is None else (ref[k][:n], unit[k][:n])
        over = ((o - r).abs() - TINY).clamp_min(0)
        ratio = torch.where(over == 0, torch.zeros_like(over), over / un)
        res[k] = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    return res


def _judge(name, out, data, t, sumsq, hp, max_norm, n=None):
    """Assert ``out`` (p, m, v) within T x unit + 2^-126 of the float64 step of ``data``, every element, with
    T = MARGIN x the fp32 CPU floor of this very case on this very data; prints both."""
    ref, unit = _ref64(data, t, sumsq, hp, max_norm)
    floor = _ratios(_emulate32(data, t, sumsq, hp, max_norm), ref, unit)
    got = _ratios(out, ref, unit, n)
    T = {k: MARGIN * floor[k] for k in floor}
    print(f"OPT-RATIO | {name} | b2 {hp[2]} t {t} sumsq {sumsq:g} max_norm {max_norm:g} | "
          + " | ".join(f"{k}: T {T[k]:.2f} err/bound {got[k] / T[k] if T[k] else got[k]:.3f}" for k in ("m", "v", "p")))
    for k in ("m", "v", "p"):
        assert got[k] <= T[k], (f"{name}: {k} needs T = {got[k]:.3f} > {T[k]:.3f} = {MARGIN:g} x the fp32 floor "
                                f"{floor[k]:.3f} (b2 {hp[2]}, t {t}, sumsq {sumsq:g}, max_norm {max_norm:g})")
    return got, T


# ------------------------------------------------------------------------------------------- self-checks

@pytest.mark.parametrize("hp_i", [0, 1])
def test_selfcheck_floor_T(hp_i):
    """The fp32 CPU floors of every (t, clip) case on the main data, i.e. T / 4 of the GPU cases (FLOOR-T lines,
    the table of docs/NUMERICS.md): finite, and at least the one rounding of the result."""
    data, hp = _data(N_MAIN), HP[hp_i]
    for t in STEPS:
        for clip, (sumsq, max_norm) in CLIPS.items():
            if clip == "nan":
                continue
            ref, unit = _ref64(data, t, sumsq, hp, max_norm)
            f = _ratios(_emulate32(data, t, sumsq, hp, max_norm), ref, unit)
            print(f"FLOOR-T | b2 {hp[2]} t {t} clip {clip} | kappa(share 1) {_kappa(t, hp[1], hp[2]):.3g} | "
                  + " | ".join(f"{k}: floor {f[k]:.2f} T {MARGIN * f[k]:.2f}" for k in ("m", "v", "p")))
            assert all(0.5 <= f[k] < 64 for k in f), (t, clip, f)


@pytest.mark.parametrize("t", [2, 7, 1000])
def test_selfcheck_mutants_exceed_the_bound(t):
    """Every mutant, evaluated in fp32 torch on the generator's data with the clip active, needs more than 4 x the
    T of the case on at least one of m, v, p -- the margin in T cannot swallow it.

    The closest is the decay applied to the updated p at t = 2: it moves p by lr wd = 3e-5 of lr |u|, and the
    POW_ULPS ulp granted to powf(0.999, 2) move sqrt(v-hat) by as much.  Only the elements whose denominator is
    mostly eps (``share`` in ``_kappa``) tell the two apart."""
    data, hp = _data(N_MAIN), HP[0]
    sumsq, max_norm = CLIPS["active"]
    ref, unit = _ref64(data, t, sumsq, hp, max_norm)
    floor = _ratios(_emulate32(data, t, sumsq, hp, max_norm), ref, unit)
    for mutant in MUTANTS:
        need = _ratios(_emulate32(data, t, sumsq, hp, max_norm, mutant), ref, unit)
        worst = max(need[k] / (MARGIN * floor[k]) for k in need)
        print(f"MUTANT | t {t} | {mutant} | " + " | ".join(f"{k}: {need[k] / (MARGIN * floor[k]):.3g} x bound"
                                                           for k in ("m", "v", "p")))
        assert worst >= 4.0, (t, mutant, need, floor)


def test_selfcheck_old_metric_passes_three_mutants():
    """The data and metrics of test_adamw_matches_cpu (m = v = 0, one gradient three times, ``_close`` at 1e-6 on p
    and 1e-5 on v, m not compared): b1 = 0.8, a bf16-stored m and the decay on the updated p all pass them.  That
    is the recorded reason for this file."""
    n = 10_000 * 64
    p0 = _r(n, dtype=torch.float32, seed=25, dev="cpu")
    g = _r(n, dtype=torch.float32, seed=26, dev="cpu") * 0.01
    sumsq = _f32(float((g[: n // 2].double() ** 2).sum() + 0.5 * (g[n // 2:].double() ** 2).sum()))
    assert sumsq > 1.0  # the clip is active there

    def three_steps(mutant):
        st = {"p": p0, "m": torch.zeros(n), "v": torch.zeros(n)}
        for t in (1, 2, 3):
            st = _emulate32((st["p"], g, st["m"], st["v"]), t, sumsq, HP[0], 1.0, mutant)
        return st

    honest = three_steps(None)
    for mutant in MUTANTS[:3]:
        bad = three_steps(mutant)
        _close(bad["p"], honest["p"], 1e-6, f"adamw_p, {mutant}")
        _close(bad["v"], honest["v"], 1e-5, f"adamw_v, {mutant}")
    for mutant in ("m stored through bf16", "b1 = 0.8"):  # and the state they leave behind is wrong
        assert (three_steps(mutant)["m"] - honest["m"]).abs().max() > 1e-3 * honest["m"].abs().max()


# ---------------------------------------------------------------------------------- guarded device buffers

def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _guarded(t, dev, fill):
    """``t`` on the device between two margins of GUARD sentinels: (whole buffer, view of the payload)."""
    full = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype)
    full[GUARD:GUARD + t.numel()] = t.reshape(-1)
    full = full.to(dev)
    return full, full[GUARD:GUARD + t.numel()].view(t.shape)


def _margins_intact(full, fill, name):
    want = _bits(torch.full((GUARD,), fill, dtype=full.dtype, device=full.device))
    assert torch.equal(_bits(full[:GUARD]), want), f"{name}: written before the range"
    assert torch.equal(_bits(full[-GUARD:]), want), f"{name}: written past the range"


def _same_bits(a, b, name):
    assert a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{name}: bits differ"


def _mirror_is_rne(mirror, p, name):
    """mirror == bf16(p) bitwise with the CPU's round-to-nearest-even cast of the kernel's own p."""
    _same_bits(mirror.cpu(), p.cpu().to(torch.bfloat16), name)


class _Flat:
    """One guarded set of flat buffers of ``data[:n]`` and one adamw_flat launch over them."""

    def __init__(self, dev, data, n, n_mirror):
        self.n, self.nm, self.dev = n, n_mirror, dev
        self.host = [x[:n] for x in data]
        (self.P, self.p), (self.Gr, self.g), (self.M, self.m), (self.V, self.v) = (
            _guarded(x, dev, NAN) for x in self.host)
        self.MIR, self.mir = _guarded(torch.full((n,), SENT_BF16, dtype=torch.bfloat16), dev, SENT_BF16)

    def run(self, t, sumsq, hp, max_norm, **kw):
        step = torch.tensor([t], dtype=torch.int64, device=self.dev)
        ss = torch.tensor([sumsq], dtype=torch.float32, device=self.dev)
        if "enable" in kw:
            kw["enable"] = torch.tensor([kw["enable"]], dtype=torch.float32, device=self.dev)
        O.adamw_flat(self.p, self.g, self.m, self.v, self.mir if self.nm else None, self.nm, step, ss, *hp, max_norm,
                     **kw)
        torch.cuda.synchronize()
        assert int(step.item()) == t and (math.isnan(sumsq) or float(ss.item()) == _f32(sumsq))
        return self

    def check_outside(self, name):
        for full, nm in ((self.P, "p"), (self.M, "m"), (self.V, "v")):
            _margins_intact(full, NAN, f"{name} {nm}")
        _margins_intact(self.Gr, NAN, f"{name} g")
        _same_bits(self.g.cpu(), self.host[1], f"{name}: the gradient was modified")
        _margins_intact(self.MIR, SENT_BF16, f"{name} mirror")
        rest = self.mir[self.nm:]
        assert bool((rest == SENT_BF16).all()), f"{name}: mirror written past n_mirror"

    def out(self):
        return {"p": self.p, "m": self.m, "v": self.v}

    def same_as(self, other, name):
        for a, b, nm in ((self.p, other.p, "p"), (self.m, other.m, "m"), (self.v, other.v, "v"),
                         (self.mir, other.mir, "mirror")):
            _same_bits(a, b, f"{name} {nm}")


def _all_nan(out, name):
    for k, t in out.items():
        assert bool(torch.isnan(t).all()), f"{name}: {k} is not NaN everywhere on a NaN norm"


CASES = [pytest.param(h, t, c, id=f"b2_{HP[h][2]}-t{t}-{c}") for h in (0, 1) for t in STEPS for c in CLIPS]


# ------------------------------------------------------------------------------------- adamw_kernel (flat)

@gpu
@pytest.mark.parametrize("hp_i,t,clip", CASES)
def test_adamw_flat_per_element(cuda, hp_i, t, clip):
    """adamw_kernel, full grid and capped grid (max_blocks = 7: three grid-stride rounds and a partial fourth), on
    N_MAIN elements: m, v, p per element, the mirror bitwise bf16(p) up to n_mirror, nothing outside the range."""
    data, hp = _data(N_MAIN), HP[hp_i]
    sumsq, max_norm = CLIPS[clip]
    nm = 49152
    full = _Flat(cuda, data, N_MAIN, nm).run(t, sumsq, hp, max_norm)
    capped = _Flat(cuda, data, N_MAIN, nm).run(t, sumsq, hp, max_norm, max_blocks=7)
    for f, name in ((full, "adamw_kernel full grid"), (capped, "adamw_kernel capped grid")):
        f.check_outside(name)
        if clip == "nan":
            _all_nan(f.out(), name)
            assert bool(torch.isnan(f.mir[:nm].float()).all()), name
        else:
            _judge(name, f.out(), data, t, sumsq, hp, max_norm)
            _mirror_is_rne(f.mir[:nm], f.p[:nm], name + " mirror")
    if clip != "nan":
        capped.same_as(full, "capped grid against full grid")


@gpu
@pytest.mark.parametrize("n", [4, 1020, 1024, 2052, N_MAIN])
@pytest.mark.parametrize("max_blocks", [0, 1, 7])
def test_adamw_flat_sizes_and_enable(cuda, n, max_blocks):
    """Sizes below one 4-element group per thread, below a thread's second chunk, across a block, each with the
    full grid and grids capped at 1 and 7 blocks: the first n elements of the main data against the same
    reference; ``enable = 0`` leaves every buffer bit-identical and ``enable = 1`` equals no ``enable``."""
    data, hp, t = _data(N_MAIN), HP[0], 7
    sumsq, max_norm = CLIPS["active"]
    nm = max(4, (n * 3 // 4) // 4 * 4)
    name = f"adamw_kernel n {n} max_blocks {max_blocks}"
    f = _Flat(cuda, data, n, nm).run(t, sumsq, hp, max_norm, max_blocks=max_blocks)
    f.check_outside(name)
    _judge(name, f.out(), data, t, sumsq, hp, max_norm, n=n)
    _mirror_is_rne(f.mir[:nm], f.p[:nm], name + " mirror")
    on = _Flat(cuda, data, n, nm).run(t, sumsq, hp, max_norm, max_blocks=max_blocks, enable=1.0)
    on.check_outside(name + " enable 1")
    on.same_as(f, name + " enable 1")
    off = _Flat(cuda, data, n, nm).run(t, sumsq, hp, max_norm, max_blocks=max_blocks, enable=0.0)
    off.check_outside(name + " enable 0")
    for got, want, nm_ in zip((off.p, off.m, off.v), (off.host[0], off.host[2], off.host[3]), "pmv"):
        _same_bits(got.cpu(), want, f"{name} enable 0: {nm_}")
    assert bool((off.mir == SENT_BF16).all()), f"{name} enable 0: mirror written"


# --------------------------------------------------------------------- adamw_seg_kernel / adamw_tr_kernel

TR_MATS = ((200, 72), (96, 128), (64, 64), (8, 4))  # edge tiles in both directions, whole tiles, less than a tile
TR_GAPS = (4, 0, 1028)
TR_LEAD, TR_MIRRORED_REST, TR_TAIL = 64, 60, 40004  # the tail carries no mirror and spans ten segment blocks


def _tr_layout():
    offs, cur = [], TR_LEAD
    for i, (r, c) in enumerate(TR_MATS):
        offs.append(cur)
        cur += r * c + (TR_GAPS[i] if i < len(TR_GAPS) else 0)
    n_mirror = cur + TR_MIRRORED_REST
    return offs, n_mirror, n_mirror + TR_TAIL


class _Tr:
    """Guarded flat buffers with the TR_MATS weights, a guarded W^T each, and one adamw_tr launch over [lo, hi)."""

    def __init__(self, dev, lo=0, hi=None):
        self.offs, self.nm, self.n = _tr_layout()
        self.lo, self.hi, self.dev = lo, self.n if hi is None else hi, dev
        self.data = _data(self.n, seed=1)
        (self.P, self.p), (self.Gr, self.g), (self.M, self.m), (self.V, self.v) = (
            _guarded(x, dev, NAN) for x in self.data)
        self.MIR, self.mir = _guarded(torch.full((self.nm,), SENT_BF16, dtype=torch.bfloat16), dev, SENT_BF16)
        self.WT = [_guarded(torch.full((c, r), SENT_BF16, dtype=torch.bfloat16), dev, SENT_BF16) for r, c in TR_MATS]
        self.inside = [i for i, (o, (r, c)) in enumerate(zip(self.offs, TR_MATS)) if o >= lo and o + r * c <= self.hi]

    def run(self, t, sumsq, hp, max_norm):
        plan = O.adamw_tr_plan(self.lo, self.hi, [(self.offs[i], *TR_MATS[i], self.WT[i][1]) for i in self.inside])
        assert plan is not None and len(plan) == 1
        step = torch.tensor([t], dtype=torch.int64, device=self.dev)
        ss = torch.tensor([sumsq], dtype=torch.float32, device=self.dev)
        O.adamw_tr(self.p, self.g, self.m, self.v, self.mir, self.nm, plan, step, ss, *hp, max_norm)
        torch.cuda.synchronize()
        return self

    def check_outside(self, name):
        lo, hi = self.lo, self.hi
        for (full, view), host, nm in (((self.P, self.p), self.data[0], "p"), ((self.M, self.m), self.data[2], "m"),
                                       ((self.V, self.v), self.data[3], "v")):
            _margins_intact(full, NAN, f"{name} {nm}")
            _same_bits(view[:lo].cpu(), host[:lo], f"{name}: {nm} below lo")
            _same_bits(view[hi:].cpu(), host[hi:], f"{name}: {nm} above hi")
        _margins_intact(self.Gr, NAN, f"{name} g")
        _same_bits(self.g.cpu(), self.data[1], f"{name}: the gradient was modified")
        _margins_intact(self.MIR, SENT_BF16, f"{name} mirror")
        untouched = torch.ones(self.nm, dtype=torch.bool)
        untouched[lo:min(hi, self.nm)] = False
        assert bool((self.mir.cpu()[untouched] == SENT_BF16).all()), f"{name}: mirror written outside [lo, hi)"
        for i, (full, view) in enumerate(self.WT):
            _margins_intact(full, SENT_BF16, f"{name} W^T {TR_MATS[i]}")
            if i not in self.inside:
                assert bool((view == SENT_BF16).all()), f"{name}: W^T {TR_MATS[i]} outside the range was written"

    def check_mirrors(self, name, nan=False):
        lo, hi = self.lo, min(self.hi, self.nm)
        if nan:
            assert bool(torch.isnan(self.mir[lo:hi].float()).all()), f"{name}: mirror"
        else:
            _mirror_is_rne(self.mir[lo:hi], self.p[lo:hi], name + " mirror")
        for i in self.inside:
            (r, c), o, wt = TR_MATS[i], self.offs[i], self.WT[i][1]
            if nan:
                assert bool(torch.isnan(wt.float()).all()), f"{name}: W^T {(r, c)}"
            else:
                _same_bits(wt, self.mir[o:o + r * c].view(r, c).t(), f"{name} W^T {(r, c)}")


@gpu
@pytest.mark.parametrize("hp_i,t,clip", CASES)
def test_adamw_tr_per_element(cuda, hp_i, t, clip):
    """adamw_seg_kernel + adamw_tr_kernel over the whole layout (a lead segment, the four weights with gaps of 4, 0
    and 1028 elements, a mirrored rest and a mirror-less tail of ten blocks): m, v, p per element, the mirror
    bitwise bf16(p), every W^T bitwise its mirror view transposed, nothing outside."""
    hp = HP[hp_i]
    sumsq, max_norm = CLIPS[clip]
    f = _Tr(cuda).run(t, sumsq, hp, max_norm)
    name = "adamw_seg_kernel + adamw_tr_kernel"
    f.check_outside(name)
    f.check_mirrors(name, nan=clip == "nan")
    if clip == "nan":
        _all_nan({"p": f.p, "m": f.m, "v": f.v}, name)
    else:
        _judge(name, {"p": f.p, "m": f.m, "v": f.v}, f.data, t, sumsq, hp, max_norm)


@gpu
def test_adamw_tr_subrange(cuda):
    """A sub-range with lo > 0: from the end of the first weight into the middle of the 1028-element gap.  The second
    and third weights are updated and transposed; everything below lo and above hi keeps its bits, the first and
    last W^T included."""
    offs, _, _ = _tr_layout()
    lo, hi = offs[1] - TR_GAPS[0], offs[2] + 64 * 64 + 512
    hp, t = HP[0], 7
    sumsq, max_norm = CLIPS["active"]
    f = _Tr(cuda, lo, hi).run(t, sumsq, hp, max_norm)
    assert f.inside == [1, 2]
    name = f"adamw_tr [{lo}, {hi})"
    f.check_outside(name)
    f.check_mirrors(name)
    sub = tuple(x[lo:hi] for x in f.data)
    _judge(name, {"p": f.p[lo:hi], "m": f.m[lo:hi], "v": f.v[lo:hi]}, sub, t, sumsq, hp, max_norm)


# ------------------------------------------------------------------------------------------- cast_to_bf16

@gpu
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 4096])
def test_cast_to_bf16_bitwise(cuda, n):
    """cast_kernel's vector body and scalar tail on ties (to even, both ways), values one fp32 ulp either side of a
    tie, fp32 denormals, the largest finite fp32 (rounds to inf), +-0, +-inf and NaN: bitwise the CPU's
    round-to-nearest-even cast.  A NaN has no single bit pattern: those elements must be NaN."""
    special = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x00000001,
                            0x00012345, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                            0x00000000, 0x80000000, 0x7F7F8000, 0x00800000], dtype=torch.int64)
    special = special.where(special < 2 ** 31, special - 2 ** 32).to(torch.int32).view(torch.float32)
    gen = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=gen) * 10 ** (torch.rand(n, generator=gen) * 60 - 30)
    idx = torch.arange(n)
    src = torch.where(idx % 3 != 1, special[(idx + n) % special.numel()], src)  # specials in the body and in the tail
    S, s = _guarded(src, cuda, NAN)
    D, d = _guarded(torch.full((n,), SENT_BF16, dtype=torch.bfloat16), cuda, SENT_BF16)
    O.cast_to_bf16(s, d)
    torch.cuda.synchronize()
    _margins_intact(D, SENT_BF16, f"cast n {n}")
    _same_bits(s.cpu(), src, "cast: the source was modified")
    want, got = src.to(torch.bfloat16), d.cpu()
    nan = torch.isnan(want)
    assert bool(torch.isnan(got[nan]).all()), "cast: NaN lost"
    _same_bits(got[~nan], want[~nan], f"cast n {n}")


# ----------------------------------------------------------------------------------------------- the norm

SS_LENS = (1, 3, 4, 7, 4096, 100003)
SS_TABLES = {
    "six": (SS_LENS, (1.0, 0.5, 0.125, 1.0, 0.5, 0.125)),
    "six-rotated-zero": (SS_LENS, (0.5, 0.0, 1.0, 0.125, 0.0, 1.0)),
    "one-long": ((100003,), (1.0,)),
    "one-short": ((3,), (0.5,)),
    "forty": ((1, 3, 4, 7) * 9 + (4096, 100003, 4096, 7), (1.0, 0.5, 0.125, 0.0) * 10),
}
SS_GAP = 1e3


def _ss_visits(n, threads):
    """f32x4 visits of one thread to a segment of n elements shared by ``threads`` threads."""
    return math.ceil(n / 4 / threads)


def _ss_rel_bound(visits, nseg):
    """Relative error bound of a sum of positive terms from the depth of the additions any term passes through, in
    fp32 roundings: the strided visits of one thread to its longest segment (the 4-fold unrolled loop chains
    fewer), one more per segment of the table, and 24 for what does not depend on the sizes -- the square (1), the
    sums inside and across the f32x4 of one visit (5), the tail element (1), the weight (1), the wave shuffles
    (6), the four waves (3) and the fp32 result (1) make 18; the partials are summed in float64."""
    return (visits + nseg + 24) * U24


@functools.lru_cache(maxsize=None)
def _ss_table(name):
    """(flat fp32, [(offset, len, weight)], float64 weighted sum, smallest sentinel share, sentinels).  Background
    1e-3 randn; the first four and last four elements of every segment (which hold every element of a len % 4
    tail) carry 1 .. 1.05 each (distinct) of a weighted sum of about their number; gaps and weight-0 segments
    hold 1e3."""
    lens, weights = SS_TABLES[name]
    gen = torch.Generator().manual_seed(len(lens))
    segs, cur = [], 8
    for k, (n, w) in enumerate(zip(lens, weights)):
        segs.append((cur, n, w))
        cur = (cur + n + 3) // 4 * 4 + (4 if k % 2 else 0)  # every other pair of segments touches, up to the padding
    flat = torch.full((cur + 8,), SS_GAP, dtype=torch.float64)
    K = sum(min(n, 8) for (_, n, w) in segs if w > 0)
    k = 0
    for o, n, w in segs:
        if w == 0:
            continue
        seg = 1e-3 * torch.randn(n, generator=gen, dtype=torch.float64)
        for i in sorted(set(range(min(4, n))) | set(range(max(0, n - 4), n))):
            seg[i] = math.sqrt((1 + 0.05 * k / K) / w) * (-1) ** k
            k += 1
        flat[o:o + n] = seg
    assert k == K
    flat = flat.float()
    ref = sum(w * float((flat[o:o + n].double() ** 2).sum()) for o, n, w in segs)
    return flat, segs, ref, 1.0 / ref, K


def _ss_check(name, got, ref, bound):
    err = abs(got - ref) / ref
    print(f"SUMSQ | {name} | err {err:.3e} | bound {bound:.3e} | err/bound {err / bound:.3f}")
    assert err <= bound, f"{name}: {got!r} against {ref!r}: relative error {err:.3e} > {bound:.3e}"


def _ss_run_all(dev, flat, segs):
    """The three routes to sum_s w_s sum x^2 on one table: yields (name, value, relative bound)."""
    from distributed_training_compare_jax_amd.ops.reduce import GradReducer

    x = flat.to(dev)
    table = O.make_segments(segs, dev)
    maxlen = max(n for _, n, _ in segs)
    OUT, out = _guarded(torch.zeros(1), dev, NAN)
    step = torch.tensor([41], dtype=torch.int64, device=dev)
    O.sumsq_segments(x, table, out, step)
    assert int(step.item()) == 42
    first = float(out.item())
    O.sumsq_segments(x, table, out, None)
    assert int(step.item()) == 42 and float(out.item()) == first  # no counter: untouched, same sum
    _margins_intact(OUT, NAN, "sumsq_segments out")
    yield "sumsq_segments", first, _ss_rel_bound(_ss_visits(maxlen, 1024 * 256), len(segs))
    for nb in (1, 8, 37):
        PART, part = _guarded(torch.full((nb,), 5.0), dev, NAN)
        O.sumsq_partial(x, table, part)
        O.sum_finish(part, out, step)
        torch.cuda.synchronize()
        _margins_intact(PART, NAN, f"sumsq_partial part nb {nb}")
        yield (f"sumsq_partial nb {nb} + sum_finish", float(out.item()),
               _ss_rel_bound(_ss_visits(maxlen, nb * 256), len(segs)))
    assert int(step.item()) == 45
    red = GradReducer(dev, arena_mb=1)
    nbs = [1 if n < 4096 else (3 if n == 4096 else 5) for _, n, _ in segs]
    PART, part = _guarded(torch.full((sum(nbs),), 5.0), dev, NAN)
    off = 0
    for (o, n, w), nb in zip(segs, nbs):
        red.add_sumsq(x[o:o + n], w, part[off:off + nb])
        off += nb
    red.flush_all()
    O.sum_finish(part, out, None)
    torch.cuda.synchronize()
    _margins_intact(PART, NAN, "add_sumsq part")
    assert int(step.item()) == 45 and red.launches == 1
    visits = max(_ss_visits(n, nb * 256) for (_, n, _), nb in zip(segs, nbs))
    yield "GradReducer.add_sumsq + sum_finish", float(out.item()), _ss_rel_bound(visits, 1)


@gpu
@pytest.mark.parametrize("name", list(SS_TABLES))
def test_sumsq_edges(cuda, name):
    """sumsq_segments, sumsq_partial + sum_finish and GradReducer.add_sumsq on tables whose edge elements each carry
    at least 1 % of the weighted sum (the forty-segment table has 96 of them), with 1e3 in every gap: a dropped
    tail, an edge counted twice, an ignored weight or one element read too many fails by orders of magnitude."""
    flat, segs, ref, share, K = _ss_table(name)
    assert share >= 0.01 and K <= 96, (share, K)
    for route, got, bound in _ss_run_all(cuda, flat, segs):
        assert share >= 1000 * bound, (route, share, bound)
        _ss_check(f"{route} | {name}", got, ref, bound)


@gpu
def test_sumsq_dynamic_range(cuda):
    """A segment of 1e-20 values (squares below the fp32 normal range) next to one of 1e15 values: finite and within
    the bound; a segment whose squares overflow: inf, not NaN."""
    gen = torch.Generator().manual_seed(5)
    n = 4096
    flat = torch.cat([1e-20 * (1 + torch.rand(n, generator=gen)), 1e15 * (1 + torch.rand(n, generator=gen))])
    segs = [(0, n, 1.0), (n, n, 0.5)]
    ref = sum(w * float((flat[o:o + k].double() ** 2).sum()) for o, k, w in segs)
    for route, got, bound in _ss_run_all(cuda, flat, segs):
        assert math.isfinite(got), route
        _ss_check(f"{route} | 1e-20 next to 1e15", got, ref, bound)
    flat = torch.cat([flat, 1e20 * (1 + torch.rand(n, generator=gen))])
    for route, got, _ in _ss_run_all(cuda, flat, segs + [(2 * n, n, 1.0)]):
        assert got == float("inf"), f"{route}: {got!r} on overflowing squares"


# ------------------------------------------------------------------------------------ FusedAdamW end to end

E2E_STEPS = 6


def _make_fused(dev):
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, model_config_from_preset
    from distributed_training_compare_jax_amd.models.params import stage_param_specs
    from distributed_training_compare_jax_amd.ops.reduce import GradReducer
    from distributed_training_compare_jax_amd.parallel.buffers import FlatParams
    from distributed_training_compare_jax_amd.train.optimizer import FusedAdamW

    cfg = model_config_from_preset("tiny", vocab_size=1000)
    layers = range(cfg.n_layers)
    flat = FlatParams(stage_param_specs(cfg, layers, True, True), 0, 1, dev, compute_dtype=torch.bfloat16)
    flat.enable_transposed([f"h.{l}.{n}.w" for l in layers for n in ("fc1", "qkv", "out")] + ["lm_head.w"])
    assert len(flat.mirror_t) == 3 * cfg.n_layers + 1
    p0, _, m0, v0 = _data(flat.numel, seed=2)
    flat.params.copy_(p0)
    flat.exp_avg.copy_(m0)
    flat.exp_avg_sq.copy_(v0)
    opt = FusedAdamW(flat, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), None)
    names = list(flat.slots)
    cuts = [flat.range_of([n for n in names if n.startswith(("lm_head", "lnf"))])[1]]
    cuts += [flat.range_of([n for n in names if n.startswith(f"h.{l}.")])[1] for l in reversed(layers)]
    assert len(cuts) == 3 and cuts == sorted(cuts) and cuts[-1] < flat.numel
    opt.set_chunks(cuts + [flat.numel])
    fused = [(flat.slots[n].offset, flat.slots[n].numel) for n in ("h.1.fc1.w", "h.0.qkv.w")]
    part = opt.set_fused_sumsq(fused, 5)
    if dev.type == "cuda":
        opt.reducer = GradReducer(dev, arena_mb=1)
    return opt, cuts, sorted(fused), part


def _e2e_grads(numel, k, cuts, fused):
    """Step k's gradient: the generator's g with the four elements either side of every cut and of every fused-range
    edge carrying 1 .. 1.25 against a background of 5 in all (each at least 1.4 % of the sum), scaled to a norm of
    0.5 (even k: no clip) or 30 (odd k: clip active)."""
    g = _data(numel, seed=10 + k)[1].double()
    g *= math.sqrt(5.0 / float((g * g).sum()))
    edges = list(cuts) + [e for o, n in fused for e in (o, o + n)]
    pos = [e + d for e in edges for d in range(-4, 4)]
    assert len(set(pos)) == len(pos) == 56
    for j, i in enumerate(pos):
        g[i] = math.sqrt(1 + 0.25 * j / len(pos)) * (-1) ** j
    g *= (0.5 if k % 2 == 0 else 30.0) / math.sqrt(float((g * g).sum()))
    return g.float()


def _fused_state(opt):
    f = opt.flat
    return [t.detach().cpu().clone() for t in (f.params, f.exp_avg, f.exp_avg_sq, f.mirror, f._mirror_t_buf, opt.sumsq)]


@pytest.mark.parametrize("where", ["cpu", pytest.param("gpu", marks=gpu)])
def test_fused_adamw_end_to_end(request, where):
    """FusedAdamW on the ``tiny`` preset's flat buffers (bf16 mirror, W^T of fc1 / qkv / out_proj / lm_head), norm
    chunks at three layer-boundary cuts, two weight ranges whose partials the test supplies from float64, on the
    GPU a GradReducer: six steps.  ``cpu`` holds the torch branch of ops/optim.py to the same float64 reference.

    Each step: the norm against the float64 sum over exactly the non-fused ranges plus the supplied partials; p, m,
    v against the float64 step of the state the optimizer held before it (nothing compounds); mirror and W^T
    bitwise; the step counter.  A second run of two steps through ``update_range(max_blocks=1)`` (the two-pass
    path: adamw_kernel, then the batched transpose) leaves bitwise the same state."""
    dev = torch.device("cpu") if where == "cpu" else request.getfixturevalue("cuda")
    opt, cuts, fused, part = _make_fused(dev)
    flat, cfg = opt.flat, opt.cfg
    hp = (cfg.lr, cfg.b1, cfg.b2, cfg.eps, cfg.weight_decay)
    in_fused = torch.zeros(flat.numel, dtype=torch.bool)
    for o, n in fused:
        in_fused[o:o + n] = True
    share = torch.tensor([0.1, 0.2, 0.3, 0.25, 0.15], dtype=torch.float64)
    # one reducer block streams at most 16384 elements (set_chunks), 256 threads, one segment per task
    ss_bound = _ss_rel_bound(_ss_visits(16384, 256), 1)
    saved, partials = {}, {}
    for k in range(1, E2E_STEPS + 1):
        g = _e2e_grads(flat.numel, k, cuts, fused)
        flat.grads.copy_(g)
        partials[k] = (share * float((g[in_fused].double() ** 2).sum())).float()
        part.copy_(partials[k])
        before = tuple(t.detach().cpu().clone() for t in (flat.params, flat.grads, flat.exp_avg, flat.exp_avg_sq))
        opt.step()
        assert int(opt.step_t.item()) == k
        ss = float(opt.sumsq.item())
        ref_ss = float((g[~in_fused].double() ** 2).sum()) + float(partials[k].double().sum())
        _ss_check(f"FusedAdamW.norm {where} step {k}", ss, ref_ss, ss_bound)
        assert abs(opt.grad_norm() - math.sqrt(ref_ss)) <= ss_bound * math.sqrt(ref_ss)
        assert (opt.grad_norm() < cfg.grad_clip) == (k % 2 == 0)
        _judge(f"FusedAdamW.step {where} step {k}", {"p": flat.params, "m": flat.exp_avg, "v": flat.exp_avg_sq},
               before, k, ss, hp, cfg.grad_clip)
        _same_bits(flat.grads.cpu(), g, "the gradient was modified")
        _mirror_is_rne(flat.mirror[:flat.n_mirror], flat.params[:flat.n_mirror], f"step {k} mirror")
        for name, (sl, wt) in flat.mirror_t.items():
            _same_bits(wt, flat._view(flat.mirror, name).t(), f"step {k} W^T {name}")
        if k <= 2:
            saved[k] = _fused_state(opt)
    if where == "gpu":
        assert opt._aw_plans.get((0, flat.numel)) is not None, "the first run must take the fused AdamW + W^T path"
    opt2, _, _, part2 = _make_fused(dev)
    for k in (1, 2):
        opt2.flat.grads.copy_(_e2e_grads(flat.numel, k, cuts, fused))
        part2.copy_(partials[k])
        opt2.norm()
        opt2.update_range(0, flat.numel, max_blocks=1)
        assert not opt2._aw_plans
        for a, b, nm in zip(_fused_state(opt2), saved[k], ("p", "m", "v", "mirror", "W^T", "sumsq")):
            _same_bits(a, b, f"two-pass path, step {k}: {nm}")
