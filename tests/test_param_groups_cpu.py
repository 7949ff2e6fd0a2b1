"""``OptimConfig.param_groups`` and the ``warmup_linear`` / ``wsd`` schedules on the CPU: the schema, the group table
built from real layouts, ``lr_at``, one engine step judged per parameter against a float64 step with that parameter's
own (weight decay, rate), a frozen group, the gloo layouts and checkpoints."""

import math
import os
import tempfile
from dataclasses import replace

import numpy as np
import pytest
import torch

import test_optimizer_scale_gpu as S
import test_parallel_cpu as P
from distributed_training_compare_jax_amd.config.schema import (OptimConfig, ParamGroup, TrainConfig,
                                                                model_config_from_preset)
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.params import all_param_specs, stage_param_specs
from distributed_training_compare_jax_amd.ops import optim as O
from distributed_training_compare_jax_amd.parallel.buffers import FlatParams
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.train.optimizer import group_table
from distributed_training_compare_jax_amd.utils import checkpoint as C

LR = 3e-3
MASK = [dict(match=["*.b", "*.g"], weight_decay=0.0)]                       # the decay mask of every GPT recipe
MASK_SCALED = MASK + [dict(match=["wte", "wpe"], lr_scale=0.5)]
FROZEN = [dict(match=["*.b", "*.g"], lr_scale=0.0)]


def _oc(groups=(), **kw):
    return OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0, param_groups=groups, **kw)


# ---------------------------------------------------------------------------------------------------- schema

def test_groups_are_normalised_and_first_match_wins():
    oc = _oc([dict(match="*.b", weight_decay=0), dict(match=["*.b", "*.g"], lr_scale=2),
              dict(match=["wte"], weight_decay=0.3, lr_scale=0.5)])
    assert oc.param_groups == (ParamGroup(("*.b",), 0.0, None), ParamGroup(("*.b", "*.g"), None, 2.0),
                               ParamGroup(("wte",), 0.3, 0.5))
    assert all(isinstance(g, ParamGroup) and isinstance(g.match, tuple) for g in oc.param_groups)
    with pytest.raises(Exception):
        oc.param_groups[0].weight_decay = 1.0  # frozen records
    assert oc.group_of("h.3.fc1.b") == 0 and oc.group_values("h.3.fc1.b") == (0.0, 1.0)  # not group 1's scale
    assert oc.group_of("h.0.ln1.g") == 1 and oc.group_values("h.0.ln1.g") == (0.1, 2.0)
    assert oc.group_of("wte") == 2 and oc.group_values("wte") == (0.3, 0.5)
    assert oc.group_of("h.0.fc1.w") == -1 and oc.group_values("h.0.fc1.w") == (0.1, 1.0)
    assert replace(oc, lr=1.0).param_groups == oc.param_groups  # records pass through dataclasses.replace


def test_groups_default_is_empty():
    oc = OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0)
    assert oc.param_groups == () and oc.groups_key() == ""
    assert _oc(MASK).groups_key() != "" and _oc(MASK).groups_key() != _oc(MASK_SCALED).groups_key()
    assert _oc(MASK).groups_key() != _oc([dict(match=["*.b", "*.g"], weight_decay=0.01)]).groups_key()


@pytest.mark.parametrize("groups,offender", [
    ([dict(match=["*.b"], weight_decay=0.0, decay=1.0)], "decay"),
    ([dict(match=[], weight_decay=0.0)], "match"),
    ([dict(weight_decay=0.0)], "match"),
    ([dict(match=["*.b"], weight_decay=-0.1)], "weight_decay"),
    ([dict(match=["*.b"], weight_decay=float("nan"))], "weight_decay"),
    ([dict(match=["*.b"], lr_scale=float("inf"))], "lr_scale"),
    ([dict(match=["*.b"], lr_scale=-1.0)], "lr_scale"),
    ([dict(match=["*.b", "*.g"])], "neither"),
    ([dict(match=["wte"], lr_scale=1.0), dict(match=["*.q"])], r"param_groups\[1\]"),
])
def test_group_refusals_name_the_offender(groups, offender):
    with pytest.raises(ValueError, match=offender):
        _oc(groups)


def test_schedule_keys_of_the_existing_kinds_are_unchanged():
    assert OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0).schedule_key() == "constant:0:0:0.0"
    oc = OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0, lr_schedule="warmup_cosine", lr_warmup_steps=3,
                     lr_decay_steps=8, lr_min_ratio=0.1)
    assert oc.schedule_key() == "warmup_cosine:3:8:0.1"
    assert _oc(lr_schedule="wsd", lr_warmup_steps=3, lr_decay_steps=20, lr_cooldown_steps=5,
               lr_min_ratio=0.1).schedule_key() == "wsd:3:20:0.1:5"
    assert _oc(lr_schedule="warmup_linear", lr_warmup_steps=3, lr_decay_steps=20).schedule_key().endswith(":17")


@pytest.mark.parametrize("kw", [
    dict(lr_schedule="linear"),
    dict(lr_schedule="wsd", lr_warmup_steps=3, lr_decay_steps=20),                           # C = 0
    dict(lr_schedule="wsd", lr_warmup_steps=3, lr_decay_steps=20, lr_cooldown_steps=18),     # W + C > N
    dict(lr_schedule="wsd", lr_warmup_steps=3, lr_decay_steps=20, lr_cooldown_steps=-1),
    dict(lr_schedule="warmup_linear", lr_warmup_steps=5, lr_decay_steps=5),
])
def test_schedule_refusals(kw):
    with pytest.raises(ValueError):
        _oc(**kw)


def test_engine_refuses_a_pattern_that_matches_nothing():
    with pytest.raises(ValueError, match=r"\*\.bias"):
        _engine(_oc([dict(match=["*.b", "*.bias"], weight_decay=0.0)]))
    with pytest.raises(ValueError, match="h.7.fc1.w"):  # tiny has two layers
        _engine(_oc([dict(match=["h.7.fc1.w"], lr_scale=0.5)]))


def test_preset_file_loads():
    from distributed_training_compare_jax_amd.config.schema import _filter_fields, load_yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    oc = OptimConfig(**_filter_fields(OptimConfig, load_yaml(os.path.join(root, "configs", "optim_config_gpt3.yaml"))))
    assert oc.b2 == 0.95 and oc.lr_schedule == "warmup_cosine"
    assert oc.group_values("h.0.ln1.g") == (0.0, 1.0) and oc.group_values("lm_head.b") == (0.0, 1.0)
    assert oc.group_values("h.0.qkv.w") == (oc.weight_decay, 1.0) and oc.group_values("wte") == (oc.weight_decay, 1.0)
    oc.check_groups([s.name for s in all_param_specs(model_config_from_preset("tiny", vocab_size=1000))])


# ----------------------------------------------------------------------------------------------------- table

def _flat(preset, layers=None, embed=True, head=True, vocab=1000):
    mc = model_config_from_preset(preset, vocab_size=vocab)
    layers = range(mc.n_layers) if layers is None else layers
    # device "meta": the layout only (gpt2-small's buffers are never allocated)
    return mc, FlatParams(stage_param_specs(mc, layers, embed, head), 0, 1, "meta", compute_dtype=torch.float32)


def _host_table(flat, oc):
    """The table without device tensors (the layout tests run on meta buffers)."""
    real = flat.device
    flat.device = torch.device("cpu")
    try:
        return group_table(flat, oc)
    finally:
        flat.device = real


@pytest.mark.parametrize("preset", ["tiny", "gpt2-small"])
def test_table_of_the_decay_mask(preset):
    oc = _oc(MASK)
    mc, flat = _flat(preset)
    tab = _host_table(flat, oc)
    runs = tab.runs
    assert runs[0][0] == 0 and runs[-1][1] == flat.numel
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])), "the runs tile [0, numel)"
    assert all(lo % 64 == 0 and hi % 64 == 0 and lo < hi for lo, hi, _, _ in runs)
    assert all(a[2:] != b[2:] for a, b in zip(runs, runs[1:])), "neighbouring runs differ"
    assert len(runs) == 2 + 8 * mc.n_layers + 1
    for name, slot in flat.slots.items():
        lo, hi, wd, s = tab.values_at(slot.offset)
        assert slot.offset + slot.numel <= hi, f"{name} straddles a run bound"
        assert (wd, s) == oc.group_values(name) == ((0.0, 1.0) if name.endswith((".b", ".g")) else (0.1, 1.0)), name
    assert tab.ends.tolist() == [r[1] for r in runs]
    assert torch.equal(tab.hp, torch.tensor([[r[2], r[3]] for r in runs], dtype=torch.float32))
    assert tab.clip(4, 68) == [(4, 68, *runs[0][2:])]  # a slice inside the first run (lm_head.w)


def test_table_counts_at_12_and_24_layers():
    for preset, want in (("gpt2-small", 99), ("gpt2-medium", 195)):
        _, flat = _flat(preset)
        assert len(_host_table(flat, _oc(MASK)).runs) == want


def test_identity_groups_collapse_to_one_run():
    _, flat = _flat("tiny")
    tab = _host_table(flat, _oc([dict(match=["*.b"], weight_decay=0.1), dict(match=["wte"], lr_scale=1.0)]))
    assert tab.runs == [(0, flat.numel, 0.1, 1.0)]
    assert group_table(flat, _oc()) is None


def test_pp2_stage_table_is_the_restriction_of_the_whole():
    oc = _oc(MASK_SCALED)
    mc, whole = _flat("tiny")
    wt = _host_table(whole, oc)
    for layers, embed, head in ((range(0, 1), True, False), (range(1, 2), False, True)):
        _, st = _flat("tiny", layers, embed, head)
        tab = _host_table(st, oc)
        for name, slot in st.slots.items():
            mine, theirs = tab.values_at(slot.offset), wt.values_at(whole.slots[name].offset)
            assert mine[2:] == theirs[2:] == oc.group_values(name), name
        # a stage's runs are the whole model's over the same parameters: the same sequence of values
        names = list(st.slots)
        seq = [wt.values_at(whole.slots[n].offset)[2:] for n in names]
        dedup = [v for i, v in enumerate(seq) if i == 0 or seq[i - 1] != v]
        assert [r[2:] for r in tab.runs] == dedup


def test_table_asserts_alignment():
    with pytest.raises(AssertionError):
        O.GroupTable([(0, 32, 0.1, 1.0), (32, 128, 0.0, 1.0)], 128, "cpu")
    with pytest.raises(AssertionError):
        O.GroupTable([(0, 64, 0.1, 1.0)], 128, "cpu")
    tab = O.GroupTable([(0, 64, 0.1, 1.0), (64, 128, 0.0, 1.0)], 128, "cpu")
    z = torch.zeros(8)
    with pytest.raises(AssertionError):  # a launch starts at a 4-aligned offset
        O.adamw_flat(z, z, z, z, None, 0, torch.ones(1, dtype=torch.int64), torch.ones(1), LR, 0.9, 0.999, 1e-8, 0.1,
                     1.0, groups=tab, base=2)
    with pytest.raises(AssertionError):  # and stays inside the table
        O.adamw_flat(z, z, z, z, None, 0, torch.ones(1, dtype=torch.int64), torch.ones(1), LR, 0.9, 0.999, 1e-8, 0.1,
                     1.0, groups=tab, base=124)


# ----------------------------------------------------------------------------------------------------- lr_at

W_, N_, C_, R_ = 3, 20, 5, 0.1


def _wsd(**kw):
    return _oc(**dict(dict(lr_schedule="wsd", lr_warmup_steps=W_, lr_decay_steps=N_, lr_cooldown_steps=C_,
                           lr_min_ratio=R_), **kw))


def _wsd_formula(c, W, N, C, r):
    if c < W:
        return LR * c / W
    if c < N - C:
        return LR
    if c < N:
        return LR * (1 - (1 - r) * (c - (N - C)) / C)
    return LR * r


C_POINTS = (0, W_ - 1, W_, N_ - C_ - 1, N_ - C_, N_ - 1, N_, N_ + 5)


def test_wsd_lr_at():
    oc = _wsd()
    for c in C_POINTS:
        assert oc.lr_at(c + 1) == pytest.approx(_wsd_formula(c, W_, N_, C_, R_), rel=1e-15, abs=0.0), c
    assert oc.lr_at(1) == 0.0
    assert oc.lr_at(W_ + 1) == LR == oc.lr_at(N_ - C_) == oc.lr_at(N_ - C_ + 1)  # the plateau, both ends, exactly
    assert oc.lr_at(N_ + 1) == pytest.approx(LR * R_, rel=1e-15) and oc.lr_at(N_ + 6) == oc.lr_at(N_ + 1)
    # continuity at both joints: one step off the plateau moves the rate by one step of the neighbouring line
    assert LR - oc.lr_at(W_) == pytest.approx(LR / W_, rel=1e-12)
    assert LR - oc.lr_at(N_ - C_ + 2) == pytest.approx(LR * (1 - R_) / C_, rel=1e-12)
    assert oc.lr_at(N_) - oc.lr_at(N_ + 1) == pytest.approx(LR * (1 - R_) / C_, rel=1e-9)


def test_warmup_linear_is_wsd_with_the_whole_decay_as_cooldown():
    lin = _oc(lr_schedule="warmup_linear", lr_warmup_steps=W_, lr_decay_steps=N_, lr_min_ratio=R_)
    twin = _wsd(lr_cooldown_steps=N_ - W_)
    assert lin.cooldown == N_ - W_ == twin.cooldown
    for t in range(1, N_ + 8):
        assert lin.lr_at(t) == twin.lr_at(t), t  # exactly: the same arithmetic
    for c in (0, W_ - 1, W_, N_ - 1, N_, N_ + 5):
        assert lin.lr_at(c + 1) == pytest.approx(_wsd_formula(c, W_, N_, N_ - W_, R_), rel=1e-15, abs=0.0)
    s1, s2 = O.LrSchedule(lin, "cpu"), O.LrSchedule(twin, "cpu")
    assert s1._args() == (s1.out.data_ptr(),) + s2._args()[1:] and s1.kind == 1


# ---------------------------------------------------------------------------------------------------- engine

def _engine(oc, out="/tmp/unused", **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1000, output_dir=out, device="cpu",
                     warmup_steps=0, dtype="fp32", **kw)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo")), mc


def _data(mc):
    return get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)


def _steps(eng, mc, it, n):
    for _ in range(n):
        eng.set_batch(next(it))
        eng.run_step()
        eng.loss_value()


def judge_per_parameter(name, flat, oc, before, t, sumsq, lr_t=None):
    """Every parameter's p, m, v against the float64 step (``S._ref64``) of the state ``before`` = (p, g, m, v) with
    that parameter's own decay and rate fp32(lr_t) * fp32(scale), at ``S._judge``'s bound: four times the fp32 CPU
    floor of the same case on the same data."""
    lr_t = oc.lr if lr_t is None else lr_t
    for pname, slot in flat.slots.items():
        wd, s = oc.group_values(pname)
        lr = float(np.float32(lr_t) * np.float32(s))
        sl = slice(slot.offset, slot.offset + slot.numel)
        data = tuple(x[sl].detach().cpu() for x in before)
        out = {"p": flat.params[sl], "m": flat.exp_avg[sl], "v": flat.exp_avg_sq[sl]}
        S._judge(f"{name} {pname}", out, data, t, sumsq, (lr, oc.b1, oc.b2, oc.eps, wd), oc.grad_clip)


def test_cpu_engine_step_per_parameter_against_float64():
    oc = _oc(MASK_SCALED)
    eng, mc = _engine(oc)
    assert eng.opt.groups is not None and len(eng.opt.groups.runs) == 2 + 8 * mc.n_layers + 1
    f = eng.flat
    p0, m0, v0 = f.params.clone(), f.exp_avg.clone(), f.exp_avg_sq.clone()
    _steps(eng, mc, _data(mc), 1)
    rec = O.last_adamw()
    assert rec["entry"] == "cpu" and rec["groups"] and rec["runs"] == len(eng.opt.groups.runs)
    g = f.grads.clone()
    assert float(g.abs().max()) > 0, "the step must leave its gradients in place for the check"
    judge_per_parameter("cpu engine", f, oc, (p0, g, m0, v0), 1, float(eng.opt.sumsq.item()))
    # and the groups are not a no-op: a masked bias differs from the run without groups exactly by the decay
    ref, _ = _engine(_oc())
    _steps(ref, mc, _data(mc), 1)
    assert O.last_adamw() == dict(entry="cpu", groups=False, runs=0, launches=0, n=f.numel, base=0)
    assert torch.equal(ref.flat.p("h.0.fc1.w"), f.p("h.0.fc1.w"))
    assert not torch.equal(ref.flat.p("h.0.ln1.g"), f.p("h.0.ln1.g"))  # ones: the decay moves them
    assert not torch.equal(ref.flat.p("wte"), f.p("wte"))              # half the rate


def frozen_group_check(make_engine, steps=1):
    """``lr_scale: 0`` on the biases and gains: they keep every bit of their initial value; every other parameter is
    ``torch.equal`` to the run without groups.  Shared with the GPU file."""
    eng, mc = make_engine(_oc(FROZEN))
    p0 = eng.flat.params.clone()
    _steps(eng, mc, _data(mc), steps)
    ref, _ = make_engine(_oc())
    _steps(ref, mc, _data(mc), steps)
    moved = 0
    for name, slot in eng.flat.slots.items():
        sl = slice(slot.offset, slot.offset + slot.numel)
        if name.endswith((".b", ".g")):
            assert torch.equal(eng.flat.params[sl].view(torch.int32), p0[sl].view(torch.int32)), f"{name} moved"
            # (a zero-initialised bias with a non-zero gradient does move without the group)
            moved += int(not torch.equal(ref.flat.params[sl], p0[sl]))
        else:
            assert torch.equal(eng.flat.params[sl], ref.flat.params[sl]), name
            assert not torch.equal(eng.flat.params[sl], p0[sl]), f"{name} did not train"
    assert moved > 0
    assert not torch.equal(eng.flat.exp_avg, torch.zeros_like(eng.flat.exp_avg))  # the Adam state still moves
    return eng, ref


def test_frozen_group_keeps_its_bits():
    frozen_group_check(_engine)


# ------------------------------------------------------------------------------------------------ gloo parity

def _worker(parallel, kw, out_dir):
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    torch.set_num_threads(1)
    mc, tc, oc = P._cfgs(parallel, **kw)
    oc = replace(oc, param_groups=MASK)
    d = init_distributed("cpu")
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
    assert eng.opt.groups is not None and O.last_adamw()["groups"]
    params = {n: eng.flat.p(n).clone() for n in eng.flat.slots}
    torch.save({"losses": r["history"], "params": params, "mesh": (eng.mesh.dp, eng.mesh.tp, eng.mesh.pp),
                "tp_idx": eng.mesh.tp_idx, "dp_idx": eng.mesh.dp_idx, "pp_idx": eng.mesh.pp_idx,
                "sp": eng.stage.sp, "head_part": eng.stage.layout.head_part},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    destroy()


def _run(parallel, world, **kw):
    with tempfile.TemporaryDirectory() as td:
        if world == 1:
            os.environ.pop("WORLD_SIZE", None)
            os.environ.pop("RANK", None)
            _worker(parallel, kw, td)
        else:
            spawn(_worker, world, args=(parallel, kw, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(world)]


@pytest.fixture(scope="module")
def single_masked():
    return _run("dp", 1)


@pytest.mark.slow
@pytest.mark.parametrize("parallel,world,kw", [
    ("dp", 2, {"zero_stage": 1}),
    ("tp", 2, {"tp_sequence_parallel": False}),
    ("pp", 2, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "1f1b"}),
])
def test_layouts_match_single_process_under_the_decay_mask(single_masked, parallel, world, kw):
    res = _run(parallel, world, **kw)
    assert res[0]["losses"] == pytest.approx(single_masked[0]["losses"], rel=1e-4, abs=1e-4)
    full, ref = P._full_params(res), single_masked[0]["params"]
    assert set(full) == set(ref)
    for n in ref:
        a, b = full[n], ref[n]
        if n.endswith("qkv.b"):  # the key bias: see test_parallel_cpu.test_layout_matches_single_process
            a, b = a.view(3, -1)[[0, 2]], b.view(3, -1)[[0, 2]]
        assert torch.allclose(a, b, rtol=1e-3, atol=2e-5), n


# ------------------------------------------------------------------------------------------------ checkpoints

def test_resume_under_the_same_groups_and_refusal_under_others(tmp_path):
    oc = _wsd(groups=MASK_SCALED)
    eng, mc = _engine(oc, out=str(tmp_path))
    it = _data(mc)
    _steps(eng, mc, it, 2)
    C.save(eng, str(tmp_path), 2)
    _steps(eng, mc, it, 1)
    straight = eng.flat.params.clone(), eng.flat.exp_avg.clone(), eng.flat.exp_avg_sq.clone()

    eng2, _ = _engine(oc, out=str(tmp_path))
    C.load_into(eng2, str(tmp_path), 2)
    it2 = _data(mc)
    for _ in range(2):
        next(it2)
    _steps(eng2, mc, it2, 1)
    for a, b in zip(straight, (eng2.flat.params, eng2.flat.exp_avg, eng2.flat.exp_avg_sq)):
        assert torch.equal(a, b)

    for other in (replace(oc, param_groups=MASK), replace(oc, param_groups=()),
                  replace(oc, param_groups=[dict(match=["*.b", "*.g"], weight_decay=0.01)] + MASK_SCALED[1:])):
        eng3, _ = _engine(other, out=str(tmp_path))
        with pytest.raises(ValueError, match="param_groups") as e:
            C.load_into(eng3, str(tmp_path), 2)
        assert oc.groups_key() in str(e.value) and other.groups_key() in str(e.value)  # names both keys
    eng4, _ = _engine(replace(oc, lr_cooldown_steps=4), out=str(tmp_path))
    with pytest.raises(ValueError, match="lr_schedule"):
        C.load_into(eng4, str(tmp_path), 2)


def test_checkpoint_without_the_field_means_no_groups(tmp_path):
    import glob
    import json

    eng, mc = _engine(_oc(), out=str(tmp_path))
    _steps(eng, mc, _data(mc), 1)
    C.save(eng, str(tmp_path), 1)
    for path in glob.glob(os.path.join(str(tmp_path), "ckpt", "step_1", "meta_rank*.json")):
        meta = json.load(open(path))
        assert meta.pop("param_groups") == ""  # as a checkpoint from before the field
        json.dump(meta, open(path, "w"))
    eng2, _ = _engine(_oc(), out=str(tmp_path))
    C.load_into(eng2, str(tmp_path), 1)
    assert torch.equal(eng2.flat.params, eng.flat.params)
    eng3, _ = _engine(_oc(MASK), out=str(tmp_path))
    with pytest.raises(ValueError, match="param_groups"):
        C.load_into(eng3, str(tmp_path), 1)


def test_metrics_record_the_number_of_groups(tmp_path):
    import json

    from distributed_training_compare_jax_amd.train.loop import train

    mc = model_config_from_preset("tiny", vocab_size=1000)
    for groups, want in ((MASK_SCALED, 2), ((), None)):
        out = str(tmp_path / f"g{len(groups)}")
        tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=2, log_every=1000, output_dir=out, device="cpu",
                         warmup_steps=0, dtype="fp32")
        train(tc, mc, _oc(groups), DistInfo(0, 1, 0, torch.device("cpu"), "gloo"), quiet=True)
        assert json.load(open(os.path.join(out, "metrics.json"))).get("param_groups") == want


_ = math
