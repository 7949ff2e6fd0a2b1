"""``OptimConfig.param_groups`` and the ``wsd`` / ``warmup_linear`` schedules on the HIP path.

The grouped kernels are pinned two ways on the rig of ``tests/test_optimizer_scale_gpu.py`` (decade-spanning states,
guarded buffers): bit for bit against the UNGROUPED kernel launched once per run with that run's decay and the rate
``fp32(lr) * fp32(scale)`` (so the grouped path is exactly "the old kernel, per run"), and per element against the
float64 optax step at that file's bound of four times the fp32 CPU floor.  ``ops.optim.last_adamw()`` is asserted
wherever a table is meant to be in use, so no case passes on the ungrouped path.

Run bounds of the main buffer (4096 elements; one block of ``adamw_kernel`` covers 2048, in two 1024-element
chunks): 64 and 128 inside a block's first chunk, 1024 on the chunk boundary, 1088 inside the second chunk, 2048 on
the block boundary, 2112 inside the second block's first chunk.  Runs are as small as 64 elements, the smallest slot.
"""

import os
import tempfile
from dataclasses import replace

import numpy as np
import pytest
import torch

import test_optimizer_scale_gpu as S
import test_param_groups_cpu as G
import test_resume_gpu as R
from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.ops import optim as O
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

N_BUF = 4096
BOUNDS = (0, 64, 128, 1024, 1088, 2048, 2112, 4096)
VALUES = ((0.1, 1.0), (0.0, 1.0), (0.1, 0.5), (0.3, 0.0))  # (weight decay, rate scale), alternating over the runs
NM_CUT = 1500                                              # the mirror ends inside the run [1088, 2048)


def _runs(bounds=BOUNDS):
    return [(a, b, *VALUES[i % len(VALUES)]) for i, (a, b) in enumerate(zip(bounds, bounds[1:]))]


def _table(dev, runs, numel=None):
    return O.GroupTable(runs, runs[-1][1] if numel is None else numel, dev)


def _scalars(dev, t, sumsq):
    return (torch.tensor([t], dtype=torch.int64, device=dev), torch.tensor([sumsq], dtype=torch.float32, device=dev))


def _lr32(lr, s):
    """The rate the grouped kernel forms: one fp32 multiply of the fp32 rate by the fp32 scale."""
    return float(np.float32(lr) * np.float32(s))


def _per_run(f, runs, t, sumsq, hp, max_norm, lr_dev=False, lo=0):
    """The reference: the UNGROUPED kernel launched once per run over ``f`` (an ``S._Flat`` whose element 0 sits at
    flat offset ``lo``) with the run's decay and fp32(lr) * fp32(scale), by value or through ``lr_dev``."""
    lr, b1, b2, eps, _ = hp
    step, ss = _scalars(f.dev, t, sumsq)
    for a, b, wd, s in runs:
        a, b = max(a, lo) - lo, min(b, lo + f.n) - lo
        if b <= a:
            continue
        k = min(max(f.nm - a, 0), b - a)
        kw = {}
        lr_run = _lr32(lr, s)
        if lr_dev:
            kw["lr_dev"] = torch.tensor([lr_run], dtype=torch.float32, device=f.dev)
            lr_run = 7.0  # a wrong by-value rate: the pointer must be what is read
        O.adamw_flat(f.p[a:b], f.g[a:b], f.m[a:b], f.v[a:b], f.mir[a:] if k else None, k, step, ss, lr_run, b1, b2, eps,
                     wd, max_norm, **kw)
        assert O.last_adamw()["groups"] is False and O.last_adamw()["entry"] in ("dtc_adamw", "dtc_adamw_lr")
    torch.cuda.synchronize()
    return f


def _grouped(f, tab, t, sumsq, hp, max_norm, lr_dev=False, base=0, **kw):
    if lr_dev:
        kw["lr_dev"] = torch.tensor([np.float32(hp[0])], dtype=torch.float32, device=f.dev)
        hp = (7.0,) + tuple(hp[1:])
    # the global decay handed over is a wrong one: every element must take its run's
    f.run(t, sumsq, hp[:4] + (0.77,), max_norm, groups=tab, base=base, **kw)
    rec = O.last_adamw()
    assert rec["entry"] == "dtc_adamw_groups" and rec["groups"] and rec["runs"] == len(tab.runs), rec
    assert rec["n"] == f.n and rec["base"] == base
    return f


# ------------------------------------------------------------------------------- grouped launch = per-run launches

@pytest.mark.parametrize("lr_dev", [False, True], ids=["by_value", "lr_dev"])
@pytest.mark.parametrize("t", [2, 7])
@pytest.mark.parametrize("clip", ["inactive", "active"])
def test_grouped_launch_equals_per_run_launches(cuda, lr_dev, t, clip):
    data, hp = S._data(S.N_MAIN), S.HP[0]
    sumsq, max_norm = S.CLIPS[clip]
    runs = _runs()
    tab = _table(cuda, runs)
    ref = _per_run(S._Flat(cuda, data, N_BUF, NM_CUT), runs, t, sumsq, hp, max_norm, lr_dev)
    assert not torch.equal(ref.p.cpu(), data[0][:N_BUF])
    frozen = slice(1024, 1088)  # scale 0: the run keeps its parameters
    S._same_bits(ref.p[frozen].cpu(), data[0][frozen], "scale 0 in the reference")
    for mb in (0, 1, 7):
        got = _grouped(S._Flat(cuda, data, N_BUF, NM_CUT), tab, t, sumsq, hp, max_norm, lr_dev, max_blocks=mb)
        name = f"grouped adamw_kernel max_blocks {mb}"
        got.check_outside(name)
        got.same_as(ref, name + " against per-run launches")  # p, m, v and the mirror, up to the cut inside a run
        S._mirror_is_rne(got.mir[:NM_CUT], got.p[:NM_CUT], name + " mirror")


@pytest.mark.parametrize("base", [4, 68, 1028, 2044])
def test_subranges_that_begin_and_end_inside_runs(cuda, base):
    """The ZeRO-1 slices: a launch over [base, base + n) with the table of the whole buffer.  Lengths that cross no
    bound, one bound and three bounds (from 2044 only two bounds lie before the end of the buffer: both), and
    n = 4: the result is the slice of the whole-buffer result, nothing outside the range is written."""
    data, hp, t = S._data(S.N_MAIN), S.HP[0], 7
    sumsq, max_norm = S.CLIPS["active"]
    tab = _table(cuda, _runs())
    whole = _grouped(S._Flat(cuda, data, N_BUF, NM_CUT), tab, t, sumsq, hp, max_norm)
    above = [b for b in BOUNDS if b > base]
    ends = {base + 4}
    for k in (0, 1, 3):
        k = min(k, len(above) - 1)
        ends.add(min(base + 56, above[0]) if k == 0 else above[k - 1] + 8)
    crossed = sorted(sum(1 for b in above if b < e) for e in ends)
    assert crossed[0] == 0 and 1 in crossed and crossed[-1] == min(3, len(above) - 1), (base, sorted(ends), crossed)
    for end in sorted(ends):
        n = end - base
        nm = min(max(NM_CUT - base, 0), n)
        sub = S._Flat(cuda, tuple(x[base:] for x in data), n, nm)
        _grouped(sub, tab, t, sumsq, hp, max_norm, base=base)
        name = f"grouped adamw_kernel [{base}, {end})"
        sub.check_outside(name)
        for a, b, nm_ in ((sub.p, whole.p, "p"), (sub.m, whole.m, "m"), (sub.v, whole.v, "v")):
            S._same_bits(a, b[base:end], f"{name} {nm_}")
        S._same_bits(sub.mir[:nm], whole.mir[base:base + nm], f"{name} mirror")


@pytest.mark.parametrize("max_blocks", [0, 3])
def test_search_depth_200_runs(cuda, max_blocks):
    """200 runs of 64 elements with alternating values (n = 12800): every block's search is eight levels deep and
    its lanes step over up to 32 runs."""
    n = 12800
    data, hp, t = S._data(S.N_MAIN), S.HP[0], 7
    sumsq, max_norm = S.CLIPS["active"]
    runs = _runs(tuple(range(0, n + 1, 64)))
    assert len(runs) == 200
    ref = _per_run(S._Flat(cuda, data, n, n), runs, t, sumsq, hp, max_norm)
    got = _grouped(S._Flat(cuda, data, n, n), _table(cuda, runs), t, sumsq, hp, max_norm, max_blocks=max_blocks)
    got.check_outside("200 runs")
    got.same_as(ref, "200 runs against per-run launches")


# ------------------------------------------------------------------------------------- per element against float64

@pytest.mark.parametrize("hp_i,t,clip", S.CASES)
def test_grouped_per_element_against_float64(cuda, hp_i, t, clip):
    """Each run of the main buffer through ``S._judge`` with that run's (lr * scale, wd): four times the fp32 CPU
    floor of the case, the bound of tests/test_optimizer_scale_gpu.py."""
    data, hp = S._data(S.N_MAIN), S.HP[hp_i]
    sumsq, max_norm = S.CLIPS[clip]
    runs = _runs()
    f = _grouped(S._Flat(cuda, data, N_BUF, NM_CUT), _table(cuda, runs), t, sumsq, hp, max_norm)
    f.check_outside("grouped adamw_kernel")
    if clip == "nan":
        S._all_nan(f.out(), "grouped adamw_kernel")
        return
    S._mirror_is_rne(f.mir[:NM_CUT], f.p[:NM_CUT], "grouped adamw_kernel mirror")
    for a, b, wd, s in runs:
        S._judge(f"grouped adamw_kernel run [{a}, {b}) wd {wd} scale {s}",
                 {"p": f.p[a:b], "m": f.m[a:b], "v": f.v[a:b]}, tuple(x[a:b] for x in data), t, sumsq,
                 (_lr32(hp[0], s), hp[1], hp[2], hp[3], wd), max_norm)


# -------------------------------------------------------------------------------------- segmented and tiled kernels

# S._Tr's layout: lead [0, 64), W0 [64, 14464), gap 4, W1 [14468, 26756), W2 [26756, 30852), gap 1028,
# W3 [31880, 31912), mirrored rest to 31972, tail to 71976.  Run bounds: 14464 (between W0 and the 4-element gap),
# 31360 (inside the 1028-element gap: a segment is split), 40000 (inside the mirror-less tail).  W0 | W1, W2 | W3 lie
# in three runs.  The table ends at the next multiple of 64 past the buffer.
TR_BOUNDS = (0, 14464, 31360, 40000, 72000)


def _tr_per_run(tr, runs, t, sumsq, hp, max_norm):
    lr, b1, b2, eps, _ = hp
    step, ss = _scalars(tr.dev, t, sumsq)
    for a, b, wd, s in runs:
        b = min(b, tr.n)
        k = min(max(tr.nm - a, 0), b - a)
        O.adamw_flat(tr.p[a:b], tr.g[a:b], tr.m[a:b], tr.v[a:b], tr.mir[a:] if k else None, k, step, ss, _lr32(lr, s),
                     b1, b2, eps, wd, max_norm)
        inside = [(tr.mir[o:o + r * c].view(r, c), tr.WT[i][1]) for i, (o, (r, c)) in
                  enumerate(zip(tr.offs, S.TR_MATS)) if a <= o and o + r * c <= b]
        O.transpose_batch([(src, dst) for src, dst in inside if src.shape[1] % 8 == 0])
        for src, dst in inside:  # the batched transpose moves 16-byte vectors: the 8 x 4 weight goes through torch
            if src.shape[1] % 8:
                dst.copy_(src.t())
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("t,clip", [(2, "inactive"), (7, "active")])
def test_segmented_and_tiled_kernels_equal_per_run_two_pass(cuda, t, clip):
    hp = S.HP[0]
    sumsq, max_norm = S.CLIPS[clip]
    runs = _runs(TR_BOUNDS)
    ref = _tr_per_run(S._Tr(cuda), runs, t, sumsq, hp, max_norm)
    tr = S._Tr(cuda)
    assert tr.n <= TR_BOUNDS[-1] < tr.n + 64 and tr.offs == [64, 14468, 26756, 31880]
    tab = _table(cuda, runs)
    mats = [(tr.offs[i], *S.TR_MATS[i], tr.WT[i][1]) for i in tr.inside]
    plan = O.adamw_tr_plan(0, tr.n, mats, groups=tab)
    assert plan is not None and len(plan) == 1 and plan.grouped
    # the ungrouped plan has 4 segments (lead, the 4-element gap, the 1028 gap, the rest); two bounds split two more
    assert plan[0][0].nseg == 6 and O.adamw_tr_plan(0, tr.n, mats)[0][0].nseg == 4
    assert {round(plan[0][1].t[i].wd, 6) for i in range(4)} == {0.1, 0.0}  # the weights lie in two decays
    step, ss = _scalars(cuda, t, sumsq)
    O.adamw_tr(tr.p, tr.g, tr.m, tr.v, tr.mir, tr.nm, plan, step, ss, hp[0], hp[1], hp[2], hp[3], 0.77, max_norm)
    torch.cuda.synchronize()
    rec = O.last_adamw()
    assert rec["entry"] == "dtc_adamw_tr_groups" and rec["groups"] and rec["launches"] == 2, rec
    name = "grouped adamw_seg_kernel + adamw_tr_kernel"
    tr.check_outside(name)
    tr.check_mirrors(name)
    for a, b, nm in ((tr.p, ref.p, "p"), (tr.m, ref.m, "m"), (tr.v, ref.v, "v"), (tr.mir, ref.mir, "mirror")):
        S._same_bits(a, b, f"{name} {nm} against adamw_flat + transpose_batch per run")
    for i in tr.inside:
        S._same_bits(tr.WT[i][1], ref.WT[i][1], f"{name} W^T {S.TR_MATS[i]}")
    for a, b, wd, s in runs:
        b = min(b, tr.n)
        S._judge(f"{name} run [{a}, {b})", {"p": tr.p[a:b], "m": tr.m[a:b], "v": tr.v[a:b]},
                 tuple(x[a:b] for x in tr.data), t, sumsq, (_lr32(hp[0], s), hp[1], hp[2], hp[3], wd), max_norm)


def test_plan_with_more_segments_than_one_list_holds(cuda):
    """200 runs, no tiled weight: 200 segments go out as three lists (96 + 96 + 8), bitwise the per-run launches."""
    n, t = 12800, 7
    data, hp = S._data(S.N_MAIN), S.HP[0]
    sumsq, max_norm = S.CLIPS["active"]
    runs = _runs(tuple(range(0, n + 1, 64)))
    ref = _per_run(S._Flat(cuda, data, n, 6400), runs, t, sumsq, hp, max_norm)
    f = S._Flat(cuda, data, n, 6400)
    plan = O.adamw_tr_plan(0, n, [], groups=_table(cuda, runs))
    assert [sb.nseg for sb, _ in plan] == [96, 96, 8] and all(tb.ntasks == 0 for _, tb in plan)
    step, ss = _scalars(cuda, t, sumsq)
    O.adamw_tr(f.p, f.g, f.m, f.v, f.mir, 6400, plan, step, ss, hp[0], hp[1], hp[2], hp[3], 0.77, max_norm)
    torch.cuda.synchronize()
    assert O.last_adamw()["launches"] == 3 and O.last_adamw()["chunks"] == 3
    f.check_outside("three segment lists")
    f.same_as(ref, "three segment lists against per-run launches")


# --------------------------------------------------------------------------------------------------- identity table

def test_identity_table_is_bitwise_the_ungrouped_launch(cuda):
    data, hp, t = S._data(S.N_MAIN), S.HP[0], 7
    sumsq, max_norm = S.CLIPS["active"]
    ident = [(a, b, hp[4], 1.0) for a, b, _, _ in _runs()]
    plain = S._Flat(cuda, data, N_BUF, NM_CUT).run(t, sumsq, hp, max_norm)
    assert O.last_adamw() == dict(entry="dtc_adamw", groups=False, runs=0, launches=1, n=N_BUF, base=0)
    f = S._Flat(cuda, data, N_BUF, NM_CUT).run(t, sumsq, hp, max_norm, groups=_table(cuda, ident))
    assert O.last_adamw() == dict(entry="dtc_adamw_groups", groups=True, runs=7, launches=1, n=N_BUF, base=0)
    f.same_as(plain, "identity table against the ungrouped kernel")
    # and the segmented + tiled pair
    ident = [(a, b, hp[4], 1.0) for a, b, _, _ in _runs(TR_BOUNDS)]
    plain = S._Tr(cuda).run(t, sumsq, hp, max_norm)
    assert O.last_adamw()["entry"] == "dtc_adamw_tr" and not O.last_adamw()["groups"]
    tr = S._Tr(cuda)
    plan = O.adamw_tr_plan(0, tr.n, [(tr.offs[i], *S.TR_MATS[i], tr.WT[i][1]) for i in tr.inside],
                           groups=_table(cuda, ident))
    step, ss = _scalars(cuda, t, sumsq)
    O.adamw_tr(tr.p, tr.g, tr.m, tr.v, tr.mir, tr.nm, plan, step, ss, *hp, max_norm)
    torch.cuda.synchronize()
    assert O.last_adamw()["entry"] == "dtc_adamw_tr_groups" and O.last_adamw()["groups"]
    for a, b, nm in ((tr.p, plain.p, "p"), (tr.m, plain.m, "m"), (tr.v, plain.v, "v"), (tr.mir, plain.mir, "mirror")):
        S._same_bits(a, b, f"identity table, segmented + tiled: {nm}")
    for i in tr.inside:
        S._same_bits(tr.WT[i][1], plain.WT[i][1], f"identity table W^T {S.TR_MATS[i]}")


# ---------------------------------------------------------------------------------------- schedules on the device

LR, W_, N_, C_, R_ = 3e-3, G.W_, G.N_, G.C_, G.R_


def _sched_oc(kind, **kw):
    base = dict(lr=LR, weight_decay=0.1, grad_clip=1.0, lr_schedule=kind, lr_warmup_steps=W_, lr_decay_steps=N_,
                lr_min_ratio=R_)
    if kind == "wsd":
        base["lr_cooldown_steps"] = C_
    return OptimConfig(**dict(base, **kw))


def _emulate32(oc, t):
    """The wsd rate in fp32 numpy, term by term as the issue's table writes it: its error against float64 is the
    floor."""
    f = np.float32
    lr, r, c = f(oc.lr), f(oc.lr_min_ratio), t - 1
    w, n, cd = oc.lr_warmup_steps, oc.lr_decay_steps, oc.cooldown
    if c < w:
        return float(lr * (f(c) / f(w)))
    if c < n - cd:
        return float(lr)
    if c >= n:
        return float(lr * r)
    return float(lr * (f(1) - (f(1) - r) * (f(c - (n - cd)) / f(cd))))


def _lr_tol(oc, t):
    """The rule of tests/test_lr_schedule_gpu.py::_lr_tol: 4 x the fp32 floor, or 4 roundings where that is exact."""
    ref = oc.lr_at(t)
    return 4.0 * max(abs(_emulate32(oc, t) - ref), abs(ref) * 2.0 ** -24)


def _sched_scalar(dev, oc, t):
    sched = O.LrSchedule(oc, dev)
    step = torch.tensor([t - 1], dtype=torch.int64, device=dev)
    O.sum_finish(torch.zeros(8, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev),
                 step=step, sched=sched)
    assert int(step.item()) == t
    return float(sched.out.item())


@pytest.mark.parametrize("kind", ["wsd", "warmup_linear"])
def test_schedule_scalar_on_the_device(cuda, kind):
    oc = _sched_oc(kind)
    cd = oc.cooldown
    for c in (0, W_ - 1, W_, N_ - cd - 1, N_ - cd, N_ - 1, N_, N_ + 5):
        if c < 0:
            continue
        got, ref = _sched_scalar(cuda, oc, c + 1), oc.lr_at(c + 1)
        print(f"LR {kind} c={c}: device {got:.9e} lr_at {ref:.9e} tol {_lr_tol(oc, c + 1):.2e}")
        assert abs(got - ref) <= _lr_tol(oc, c + 1), (kind, c, got, ref)
        if W_ <= c <= N_ - cd:
            assert got == float(np.float32(LR)), (kind, c, got)  # the plateau (its last point is the line's first)
    assert _sched_scalar(cuda, oc, 1) == 0.0


def test_warmup_linear_and_its_wsd_twin_agree_bit_for_bit(cuda):
    lin, twin = _sched_oc("warmup_linear"), _sched_oc("wsd", lr_cooldown_steps=N_ - W_)
    for t in range(1, N_ + 7):
        a, b = _sched_scalar(cuda, lin, t), _sched_scalar(cuda, twin, t)
        assert np.float32(a).tobytes() == np.float32(b).tobytes(), (t, a, b)
    # both kernels' sum + schedule entry points
    x = torch.ones(64, device=cuda)
    sched = O.LrSchedule(lin, cuda)
    step = torch.tensor([9], dtype=torch.int64, device=cuda)
    O.sumsq_segments(x, O.make_segments([(0, 64, 1.0)], cuda), torch.zeros(1, device=cuda), step=step, sched=sched)
    assert float(sched.out.item()) == _sched_scalar(cuda, lin, 10)


# ------------------------------------------------------------------------------------------------------- engine

IDENTITY = [dict(match=["*.b", "*.g"], weight_decay=0.1), dict(match=["wte"], lr_scale=1.0)]


def _engine(dev, oc, use_graph=True, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/x", use_graph=use_graph,
                     **kw)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, dev, "nccl")), mc


def _state(eng):
    torch.cuda.synchronize()
    f = eng.flat
    return {"params": f.params.clone(), "exp_avg": f.exp_avg.clone(), "exp_avg_sq": f.exp_avg_sq.clone(),
            "mirror": f.mirror.clone(), "mirror_t": f._mirror_t_buf.clone()}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_identity_groups_equal_no_groups(cuda, use_graph):
    out = {}
    for name, groups in (("plain", ()), ("identity", IDENTITY)):
        eng, mc = _engine(cuda, G._oc(groups), use_graph)
        G._steps(eng, mc, G._data(mc), 3)
        out[name] = _state(eng)
        rec = O.last_adamw()
        assert rec["groups"] == (name == "identity") and (eng.opt.groups is not None) == (name == "identity"), rec
        if name == "identity":
            assert rec["entry"] == "dtc_adamw_tr_groups" and eng.opt.groups.runs == [(0, eng.flat.numel, 0.1, 1.0)]
        if use_graph:
            assert eng.program.recorded and eng.program.n_graphs == 1
        eng.close()
    assert not R.state_mismatches(out["identity"], out["plain"]), R.state_mismatches(out["identity"], out["plain"])


def test_engine_frozen_group(cuda):
    eng, ref = G.frozen_group_check(lambda oc: _engine(cuda, oc))
    assert eng.opt.groups is not None and ref.opt.groups is None  # (one step: it runs before the capture)
    assert O.last_adamw()["entry"] == "dtc_adamw_tr" and not O.last_adamw()["groups"]  # the reference ran last
    S._mirror_is_rne(eng.flat.mirror[:eng.flat.n_mirror], eng.flat.params[:eng.flat.n_mirror], "frozen group mirror")


def test_engine_decay_mask_deferred_equals_undeferred(cuda):
    out = {}
    for defer in (False, True):
        eng, mc = _engine(cuda, G._oc(G.MASK), defer_optimizer=defer)
        G._steps(eng, mc, G._data(mc), 3)
        eng.flush_optimizer()
        out[defer] = _state(eng)
        assert bool(eng.defer_opt) == defer and O.last_adamw()["groups"]
        if defer:  # the capped-grid launches of the deferred update went through the table
            assert O.last_adamw()["entry"] == "dtc_adamw_groups", O.last_adamw()
        eng.close()
    assert not R.state_mismatches(out[True], out[False]), R.state_mismatches(out[True], out[False])


def test_engine_wsd_with_groups_resumes_bitwise(cuda):
    """A (3 steps), B (2 steps and a checkpoint), C (resumed, 1 step) under wsd (the checkpoint falls on the
    cooldown) and the decay mask plus a scaled group: B's losses followed by C's are A's, and C ends on A's state."""
    from distributed_training_compare_jax_amd.train.loop import train

    oc = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0, lr_schedule="wsd", lr_warmup_steps=1, lr_decay_steps=4,
                     lr_cooldown_steps=3, lr_min_ratio=0.1, param_groups=G.MASK_SCALED)

    def run(out_dir, **kw):
        tc = TrainConfig(seed=0, parallel="dp", batch=4, log_every=1000, output_dir=out_dir, device="cuda",
                         warmup_steps=0, **kw)
        return R._snap(train(tc, R._mc(), oc, DistInfo(0, 1, 0, cuda, "nccl"), quiet=True, write_csv=False))

    ck = R._tmpdir()
    a = run(R._tmpdir(), steps=3)
    b = run(ck, steps=2, ckpt_every=2)
    c = run(ck, steps=1, resume=True)
    assert a["live"]["sched"] and a["live"]["graphs"] >= 1 and a["live"]["mirror_t"] > 0
    R.assert_same_run(b["history"] + c["history"], a["history"], c["state"], a["state"], "wsd + groups: B + C against A")
    assert c["lr"] == a["lr"] and b["lr"] != a["lr"] and 0 < a["lr"] < 3e-3, (a["lr"], b["lr"], c["lr"])
    other = replace(oc, param_groups=G.MASK)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, log_every=1000, output_dir=ck, device="cuda", warmup_steps=0,
                     steps=1, resume=True)
    with pytest.raises(ValueError, match="param_groups"):
        train(tc, R._mc(), other, DistInfo(0, 1, 0, cuda, "nccl"), quiet=True, write_csv=False)


# ------------------------------------------------------------------------------------------ FusedAdamW end to end

def test_fused_adamw_end_to_end_with_groups(cuda):
    """``S.test_fused_adamw_end_to_end``'s set-up (the ``tiny`` layout, bf16 mirror, W^T, norm chunks, synthetic
    decade-spanning gradients) under the decay mask plus a scaled group, 3 steps on the GPU: every parameter against
    the float64 optax step of its run; mirror and W^T bitwise."""
    from distributed_training_compare_jax_amd.models.params import stage_param_specs
    from distributed_training_compare_jax_amd.ops.reduce import GradReducer
    from distributed_training_compare_jax_amd.parallel.buffers import FlatParams
    from distributed_training_compare_jax_amd.train.optimizer import FusedAdamW

    mc = model_config_from_preset("tiny", vocab_size=1000)
    layers = range(mc.n_layers)
    flat = FlatParams(stage_param_specs(mc, layers, True, True), 0, 1, cuda, compute_dtype=torch.bfloat16)
    flat.enable_transposed([f"h.{l}.{n}.w" for l in layers for n in ("fc1", "qkv", "out")] + ["lm_head.w"])
    p0, _, m0, v0 = S._data(flat.numel, seed=2)
    flat.params.copy_(p0)
    flat.exp_avg.copy_(m0)
    flat.exp_avg_sq.copy_(v0)
    oc = OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0, param_groups=G.MASK_SCALED)
    opt = FusedAdamW(flat, oc, None)
    opt.reducer = GradReducer(cuda, arena_mb=1)
    assert len(opt.groups.runs) == 2 + 8 * mc.n_layers + 1
    for k in (1, 2, 3):
        g = S._data(flat.numel, seed=10 + k)[1].double()
        g = (g * ((0.5 if k % 2 == 0 else 30.0) / float((g * g).sum()) ** 0.5)).float()
        flat.grads.copy_(g)
        before = tuple(t.detach().cpu().clone() for t in (flat.params, flat.grads, flat.exp_avg, flat.exp_avg_sq))
        opt.step()
        torch.cuda.synchronize()
        rec = O.last_adamw()
        assert rec["entry"] == "dtc_adamw_tr_groups" and rec["groups"] and rec["runs"] == len(opt.groups.runs), rec
        assert int(opt.step_t.item()) == k and (opt.grad_norm() < oc.grad_clip) == (k % 2 == 0)
        G.judge_per_parameter(f"FusedAdamW + groups step {k}", flat, oc, before, k, float(opt.sumsq.item()))
        S._mirror_is_rne(flat.mirror[:flat.n_mirror], flat.params[:flat.n_mirror], f"step {k} mirror")
        for name, (sl, wt) in flat.mirror_t.items():
            S._same_bits(wt, flat._view(flat.mirror, name).t(), f"step {k} W^T {name}")
    # the two-pass path (adamw_kernel with the table, then the batched transpose) leaves the same bits
    flat2 = FlatParams(stage_param_specs(mc, layers, True, True), 0, 1, cuda, compute_dtype=torch.bfloat16)
    flat2.enable_transposed(list(flat.mirror_t))
    flat2.params.copy_(before[0])
    flat2.exp_avg.copy_(before[2])
    flat2.exp_avg_sq.copy_(before[3])
    flat2.grads.copy_(before[1])
    opt2 = FusedAdamW(flat2, oc, None)
    opt2.step_t.fill_(2)
    opt2.norm()
    opt2.update_range(0, flat2.numel, max_blocks=1)
    torch.cuda.synchronize()
    assert O.last_adamw()["entry"] == "dtc_adamw_groups" and not opt2._aw_plans
    for a, b, nm in ((flat2.params, flat.params, "p"), (flat2.exp_avg, flat.exp_avg, "m"),
                     (flat2.exp_avg_sq, flat.exp_avg_sq, "v"), (flat2.mirror, flat.mirror, "mirror"),
                     (flat2._mirror_t_buf, flat._mirror_t_buf, "W^T")):
        S._same_bits(a, b, f"two-pass path with the table: {nm}")


# ------------------------------------------------------------------------------------------ two ranks on one GPU

def _dp_worker(kw, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    kw = dict(kw)
    clip = kw.pop("grad_clip")
    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=4, log_every=1000, output_dir="/tmp/unused", device="cuda",
                     warmup_steps=2, dp_bucket_mb=0.25, dp_tail_mb=0.05, **kw)
    d = init_distributed("cuda")
    oc = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=clip, param_groups=G.MASK)
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
    eng.check_health()
    torch.save({"losses": r["history"], "graphs": r["n_graphs"], "comms": r["n_comms"], "last": O.last_adamw(),
                "runs": len(eng.opt.groups.runs), "params": eng.flat.params.cpu(),
                "named": {n: eng.flat.p(n).detach().float().cpu().clone() for n in eng.flat.slots},
                "dp_idx": eng.mesh.dp_idx, "tp_idx": eng.mesh.tp_idx},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


def _spawn(world, kw):
    with tempfile.TemporaryDirectory() as td:
        if world == 1:
            for k in ("WORLD_SIZE", "RANK"):
                os.environ.pop(k, None)
            _dp_worker(kw, td)
        else:
            spawn(_dp_worker, world, args=(kw, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(world)]


@pytest.mark.slow
def test_dp2_zero_p2p_with_groups_equals_replicated_p2p(cuda):
    """grad_clip 1e9: an inactive clip (the two norms differ in summation order only, and neither scales a gradient);
    the owned slices of the sharded update begin and end inside runs."""
    zero = _spawn(2, dict(zero_stage=1, zero_comm="p2p", grad_clip=1e9))
    repl = _spawn(2, dict(dp_comm="p2p", dp_embed_gather=False, grad_clip=1e9))
    for r in zero + repl:
        assert r["graphs"] == 1 and r["comms"] == 0 and r["last"]["groups"] and r["runs"] == 2 + 8 * 4 + 1, r["last"]
    assert all(r["last"]["entry"] == "dtc_adamw_groups" for r in zero)
    for a, b in zip(zero, repl):
        assert torch.equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
    assert torch.equal(zero[0]["params"], zero[1]["params"])


@pytest.mark.slow
def test_dp2_zero1_process_group_with_groups_matches_dp1(cuda):
    """``zero_stage: 1`` over the process group against one rank, both under the decay mask, at the tolerance of
    tests/test_dist_gpu.py::test_two_ranks_match_single_gpu (bf16 compute: reduction order and rounding differ, the
    optimizer trajectory must not): losses within 2e-2, every tensor's update within 15 % of the single-rank one."""
    one = _spawn(1, dict(grad_clip=1.0))
    two = _spawn(2, dict(zero_stage=1, grad_clip=1.0))
    assert all(r["last"]["groups"] for r in one + two) and two[0]["last"]["entry"] == "dtc_adamw_groups"
    assert two[0]["losses"] == pytest.approx(one[0]["losses"], rel=2e-2, abs=2e-2)
    assert torch.equal(two[0]["params"], two[1]["params"])
    mc4 = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1000, output_dir="/tmp/unused", device="cuda")
    init = Engine(mc4, tc, G._oc(G.MASK), DistInfo(0, 1, 0, cuda, "nccl"))
    for n in one[0]["named"]:
        a, b, p0 = two[0]["named"][n], one[0]["named"][n], init.flat.p(n).detach().float().cpu()
        if n.endswith("qkv.b"):  # key bias: analytically zero gradient, Adam normalises its noise
            a, b, p0 = (x.view(3, -1)[[0, 2]] for x in (a, b, p0))
        da, db = a - p0, b - p0
        err = ((da - db).norm() / (db.norm() + 1e-12)).item()
        assert err < 0.15, f"{n}: update differs from the single-rank run by {err:.3f} (relative)"
    init.close()
