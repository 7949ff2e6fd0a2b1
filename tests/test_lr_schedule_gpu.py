"""``lr_schedule: warmup_cosine`` on the HIP path: the device scalar (eager and replayed), the three AdamW kernels
reading it through their pointer, the engine under a graph / ZeRO-1 / accumulation, and the constant path against
bytes recorded at the parent commit (``tests/golden/adamw_constant_parent.npz``)."""

import functools
import math
import os
import tempfile

import numpy as np
import pytest
import torch

import test_optimizer_scale_gpu as S
from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.ops import optim as O
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_constant_parent.npz")
LR, W, N, R = 3e-3, 3, 8, 0.1


def _oc(lr=LR, **kw):
    return OptimConfig(lr=lr, weight_decay=0.1, grad_clip=1.0, lr_schedule="warmup_cosine", lr_warmup_steps=W,
                       lr_decay_steps=N, lr_min_ratio=R, **kw)


def _emulate32(oc, t):
    """The schedule in fp32 numpy, term by term as written in the issue: its error against float64 is the floor."""
    f = np.float32
    lr, r, c = f(oc.lr), f(oc.lr_min_ratio), t - 1
    w, n = oc.lr_warmup_steps, oc.lr_decay_steps
    if c < w:
        return float(lr * (f(c) / f(w)))
    x = f(min(c - w, n - w)) / f(n - w)
    return float(lr * (r + (f(1) - r) * (f(0.5) * (f(1) + np.cos(f(np.pi) * x, dtype=np.float32)))))


def _lr_tol(oc, t):
    """4 x the fp32 floor; where the emulation happens to be exact, 4 roundings of the value (the formula has more
    than four fp32 operations)."""
    ref = oc.lr_at(t)
    return 4.0 * max(abs(_emulate32(oc, t) - ref), abs(ref) * 2.0 ** -24)


def _engine(dev, oc, use_graph, batch=4, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=1, log_every=1, output_dir="/tmp/x", use_graph=use_graph,
                     **kw)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, dev, "nccl")), mc


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_device_scalar_follows_the_schedule(cuda, use_graph):
    oc = _oc()
    eng, mc = _engine(cuda, oc, use_graph)
    it = get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)
    seen = []
    for t in range(1, 13):
        eng.set_batch(next(it))
        eng.run_step()
        eng.loss_value()
        got = eng.opt.lr_value()
        seen.append(got)
        print(f"LR t={t}: device {got:.9e} lr_at {oc.lr_at(t):.9e} tol {_lr_tol(oc, t):.2e}")
        assert abs(got - oc.lr_at(t)) <= _lr_tol(oc, t), (t, got, oc.lr_at(t))
        assert int(eng.opt.step_t.item()) == t
    if use_graph:
        assert eng.program.recorded and eng.program.n_graphs == 1
        # replayed steps (t >= 3) see different rates: the value is not frozen into the graph
        assert len(set(seen[2:9])) == 7, seen
    assert seen[0] == 0.0 and seen[-1] == pytest.approx(LR * R, rel=1e-6)


# ------------------------------------------------------------------------------------ per-element parameters
def _sched_scalar(dev, oc, t):
    """The device scalar of update t, written by the norm's finishing kernel from the step counter t - 1."""
    sched = O.LrSchedule(oc, dev)
    step = torch.tensor([t - 1], dtype=torch.int64, device=dev)
    O.sum_finish(torch.zeros(8, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev),
                 step=step, sched=sched)
    assert int(step.item()) == t
    return sched.out


@pytest.mark.parametrize("t", [2, 3, 5, 7, 12])
@pytest.mark.parametrize("clip", ["inactive", "active"])
def test_kernels_read_the_scheduled_rate(cuda, t, clip):
    """adamw_kernel (full and capped grid), adamw_seg_kernel and adamw_tr_kernel with the schedule pointer against
    the float64 optax step at ``lr_at(t)``: 4 x the fp32 floor per element on the decade-spanning states of
    tests/test_optimizer_scale_gpu.py; the mirror and W^T bitwise the cast of p.  The by-value lr handed over is a
    wrong one (7.0), so a kernel that ignored the pointer fails."""
    lr0, b1, b2, eps, wd = S.HP[0]
    oc = _oc(lr=lr0)
    hp_ref = (oc.lr_at(t), b1, b2, eps, wd)
    hp_call = (7.0, b1, b2, eps, wd)
    sumsq, max_norm = S.CLIPS[clip]
    lr_dev = _sched_scalar(cuda, oc, t)
    assert abs(float(lr_dev.item()) - oc.lr_at(t)) <= _lr_tol(oc, t)
    data, nm = S._data(S.N_MAIN), 49152
    full = S._Flat(cuda, data, S.N_MAIN, nm).run(t, sumsq, hp_call, max_norm, lr_dev=lr_dev)
    capped = S._Flat(cuda, data, S.N_MAIN, nm).run(t, sumsq, hp_call, max_norm, max_blocks=7, lr_dev=lr_dev)
    for f, name in ((full, "adamw_kernel + lr pointer"), (capped, "adamw_kernel capped + lr pointer")):
        f.check_outside(name)
        S._judge(name, f.out(), data, t, sumsq, hp_ref, max_norm)
        S._mirror_is_rne(f.mir[:nm], f.p[:nm], name + " mirror")
    capped.same_as(full, "capped grid against full grid")

    tr = S._Tr(cuda)
    plan = O.adamw_tr_plan(tr.lo, tr.hi, [(tr.offs[i], *S.TR_MATS[i], tr.WT[i][1]) for i in tr.inside])
    step = torch.tensor([t], dtype=torch.int64, device=cuda)
    ss = torch.tensor([sumsq], dtype=torch.float32, device=cuda)
    O.adamw_tr(tr.p, tr.g, tr.m, tr.v, tr.mir, tr.nm, plan, step, ss, *hp_call, max_norm, lr_dev=lr_dev)
    torch.cuda.synchronize()
    name = "adamw_seg_kernel + adamw_tr_kernel + lr pointer"
    tr.check_outside(name)
    tr.check_mirrors(name)
    S._judge(name, {"p": tr.p, "m": tr.m, "v": tr.v}, tr.data, t, sumsq, hp_ref, max_norm)


def test_zero_rate_leaves_parameters_bitwise(cuda):
    """t = 1 under a warmup: lr_1 = 0, p keeps every bit while m and v move (all three kernels)."""
    lr0, b1, b2, eps, wd = S.HP[0]
    oc = _oc(lr=lr0)
    lr_dev = _sched_scalar(cuda, oc, 1)
    assert float(lr_dev.item()) == 0.0
    data = S._data(S.N_MAIN)
    f = S._Flat(cuda, data, S.N_MAIN, 0).run(1, 1.0, (7.0, b1, b2, eps, wd), 1.0, lr_dev=lr_dev)
    S._same_bits(f.p.cpu(), data[0], "p at lr 0")
    assert not torch.equal(f.m.cpu(), data[2])


# ------------------------------------------------------------------------------------------------- engine
def _run_engine(dev, oc, use_graph, n, **kw):
    eng, mc = _engine(dev, oc, use_graph, **kw)
    it = get_batch_iterator(eng.global_batch, mc.max_seq_len + 1, vocab=999)
    losses, lrs = [], []
    for _ in range(n):
        eng.set_batch(next(it))
        eng.run_step()
        losses.append(eng.loss_value())
        lrs.append(eng.opt.lr_value())
    torch.cuda.synchronize()
    return eng, losses, lrs


def test_engine_graph_matches_eager_over_scheduled_steps(cuda):
    out = {}
    for mode in (False, True):
        eng, losses, lrs = _run_engine(cuda, _oc(), mode, 6)
        out[mode] = (losses, lrs, eng.flat.params.clone())
    assert out[True][0] == pytest.approx(out[False][0], rel=1e-5, abs=1e-5), out
    assert out[True][1] == out[False][1]
    assert torch.allclose(out[True][2], out[False][2], rtol=1e-4, atol=1e-6)


def test_accumulation_advances_the_rate_once_per_update(cuda):
    oc = _oc()
    eng, losses, lrs = _run_engine(cuda, oc, True, 6, grad_accum=2)
    assert int(eng.opt.step_t.item()) == 6 and eng.program.n_graphs == 1
    for t, got in enumerate(lrs, 1):
        assert abs(got - oc.lr_at(t)) <= _lr_tol(oc, t), (t, got, oc.lr_at(t))


def _dp_worker(kw, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=6, log_every=1000, output_dir="/tmp/unused", device="cuda",
                     warmup_steps=2, dp_bucket_mb=0.25, dp_tail_mb=0.05, **kw)
    d = init_distributed("cuda")
    # grad_clip 1e9: an inactive clip (the two norms differ in summation order only, and neither scales a gradient)
    oc = OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1e9, lr_schedule="warmup_cosine", lr_warmup_steps=W,
                     lr_decay_steps=N, lr_min_ratio=R)
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
    eng.check_health()
    torch.save({"losses": r["history"], "graphs": r["n_graphs"], "comms": r["n_comms"], "lr": eng.opt.lr_value(),
                "params": eng.flat.params.cpu(), "t": int(eng.opt.step_t.item())},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


def _spawn2(kw):
    with tempfile.TemporaryDirectory() as td:
        spawn(_dp_worker, 2, args=(kw, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(2)]


@pytest.mark.slow
def test_dp2_zero_p2p_with_schedule_equals_replicated_p2p(cuda):
    zero = _spawn2(dict(zero_stage=1, zero_comm="p2p"))
    repl = _spawn2(dict(dp_comm="p2p", dp_embed_gather=False))
    oc = _oc()
    for r in zero + repl:
        assert r["graphs"] == 1 and r["comms"] == 0 and r["t"] == 8
        assert abs(r["lr"] - oc.lr_at(8)) <= _lr_tol(oc, 8)
    for a, b in zip(zero, repl):
        assert torch.equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
    assert torch.equal(zero[0]["params"], zero[1]["params"])


# ------------------------------------------------------------------------- constant path against the parent
def constant_path_outputs(dev):
    """What ``tests/golden/adamw_constant_parent.npz`` holds (recorded with this very function at the parent
    commit, so it uses nothing the parent lacks): p, m, v and the bf16 mirror after 3 default-configuration steps
    of a small engine, and the direct outputs of adamw_kernel and adamw_seg_kernel + adamw_tr_kernel."""
    mc = model_config_from_preset("tiny", vocab_size=100, n_layers=1, d_ff=128)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/x", use_graph=True)
    eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl"))
    it = get_batch_iterator(4, mc.max_seq_len + 1, vocab=99)
    for _ in range(3):
        eng.set_batch(next(it))
        eng.run_step()
        eng.loss_value()
    torch.cuda.synchronize()
    f = eng.flat
    i16 = lambda x: x.detach().cpu().view(torch.int16).numpy().copy()  # noqa: E731
    f32 = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    out = {"eng_p": f32(f.params), "eng_m": f32(f.exp_avg), "eng_v": f32(f.exp_avg_sq),
           "eng_mirror": i16(f.mirror[:f.n_mirror])}
    hp, t = S.HP[0], 7
    sumsq, max_norm = S.CLIPS["active"]
    n, nm = 2052, 1024
    fl = S._Flat(dev, S._data(S.N_MAIN), n, nm).run(t, sumsq, hp, max_norm)
    out.update(flat_p=f32(fl.p), flat_m=f32(fl.m), flat_v=f32(fl.v), flat_mirror=i16(fl.mir[:nm]))
    # adamw_seg_kernel + adamw_tr_kernel over the sub-range of test_adamw_tr_subrange (two weights, a gap, segments)
    offs, _, _ = S._tr_layout()
    lo, hi = offs[1] - S.TR_GAPS[0], offs[2] + 64 * 64 + 512
    tr = S._Tr(dev, lo, hi).run(t, sumsq, hp, max_norm)
    out.update(tr_p=f32(tr.p[lo:hi]), tr_m=f32(tr.m[lo:hi]), tr_v=f32(tr.v[lo:hi]), tr_mirror=i16(tr.mir[lo:hi]))
    for i in tr.inside:
        out[f"tr_wt{i}"] = i16(tr.WT[i][1])
    return out


def test_constant_path_reproduces_the_parent_bitwise(cuda):
    gold = np.load(GOLDEN)
    got = constant_path_outputs(cuda)
    assert set(gold.files) == set(got)
    for k in gold.files:
        a, b = gold[k], got[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        same = a.view(np.uint8) == b.view(np.uint8)
        assert same.all(), f"{k}: {int((~same).sum())} bytes differ from the parent commit's"


_ = functools, math
