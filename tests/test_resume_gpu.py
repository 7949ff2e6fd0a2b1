"""Checkpoint resume on the HIP path, bit for bit against the uninterrupted run.

Two identical runs agree bit for bit (``test_engine_gpu.py::test_bitwise_deterministic_training``), so the straight run
is an exact oracle for a run that stops at a checkpoint and continues in a fresh engine: every comparison here is
``==`` on the loss lists and on the bits of the flat buffers, without a tolerance.

A checkpoint holds ``params``, ``exp_avg``, ``exp_avg_sq`` and ``step_t``.  Everything else the next step reads is
rebuilt by kernels on load (the bf16 mirror, its transposed twin, the e4m3 / MXFP8 weight mirrors), is a function of
the device step counter (the Philox dropout stream, the in-graph learning-rate schedule, the fused LayerNorms' epoch),
or is engine state that must come up as the uninterrupted run has it at that step (the deferred optimizer's pending
switch, the sparse wte-gradient zeroing, the fused Σg² partials of the global norm).

Model: the tiny preset at ``d_model`` 256, 4 heads (head_dim 64), ``d_ff`` 1024, 2 layers, T 128, vocab 1000, batch 4 =
512 tokens per step: the smallest shape at which the GEMM-fused LayerNorms (``D % 256 == 0``, ``M % 128 == 0``), the
transposed mirror, the grouped weight gradients with their Σg² partials and the FP8 GEMMs (k-step 128) are all live.
``grad_clip`` 1.0 with ``lr`` 3e-3 keeps the clip factor in the update (the printed norms are above 1), which is the
path a difference in the norm's summation order takes into the parameters.

Each case runs A (6 steps), B (3 steps and a checkpoint) and C (``resume=True``, 3 steps) through ``train.loop.train``,
so ``maybe_resume``, the data iterator's ``start_step`` and the ``gstep`` accounting are under test too.  The
multi-process cases (tp2 with sequence parallelism, pp2 1f1b with a split head, dp2 on the process-group path) run
two ranks on one GPU over gloo, one ``train`` per spawn, one spawn at a time: C is a fresh process there.
"""

import atexit
import os
import shutil
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn

gpu = pytest.mark.gpu
STEPS, CKPT = 6, 3
OPT = dict(lr=3e-3, weight_decay=0.1, grad_clip=1.0)
SCHED = dict(lr_schedule="warmup_cosine", lr_warmup_steps=2, lr_decay_steps=6)
PLAIN = dict(A=dict(warmup_steps=0, steps=STEPS), B=dict(warmup_steps=0, steps=CKPT, ckpt_every=CKPT),
             C=dict(warmup_steps=0, steps=STEPS - CKPT, resume=True))
# the accounting of tests/test_zero_p2p_engine_gpu.py: warmup steps count towards the checkpoint's step
OFFSET = dict(A=dict(warmup_steps=2, steps=4), B=dict(warmup_steps=2, steps=1, ckpt_every=CKPT),
              C=dict(warmup_steps=0, steps=3, resume=True))

# name -> (TrainConfig fields, OptimConfig fields, environment, the three runs)
CASES = {
    "default": ({}, {}, {}, PLAIN),
    "fused_norm_off": ({}, {}, {"DTC_FUSED_NORM": "0"}, PLAIN),
    "eager": (dict(use_graph=False), {}, {}, PLAIN),
    "fp32": (dict(dtype="fp32"), {}, {}, PLAIN),
    "fp8": (dict(fwd_gemm_dtype="fp8"), {}, {}, PLAIN),
    "mxfp8": (dict(fwd_gemm_dtype="mxfp8"), {}, {}, PLAIN),
    "defer_optimizer": (dict(defer_optimizer=True), {}, {}, PLAIN),
    "accum_schedule": (dict(grad_accum=2), SCHED, {}, PLAIN),
    "warmup_offset": ({}, {}, {}, OFFSET),
    "eval": (dict(eval_every=CKPT, eval_batches=2), {}, {}, PLAIN),
}


def _mc(**over):
    return model_config_from_preset("tiny", vocab_size=1000, **dict(dict(d_model=256, n_heads=4, d_ff=1024, n_layers=2,
                                                                         max_seq_len=128), **over))


def _tc(case, out_dir, **run):
    return TrainConfig(seed=0, parallel="dp", batch=4, log_every=1000, output_dir=out_dir, device="cuda",
                       **dict(CASES[case][0], **run))


def _tmpdir():
    td = tempfile.mkdtemp(prefix="dtc_resume_")
    atexit.register(shutil.rmtree, td, ignore_errors=True)
    return td


# ------------------------------------------------------------------------------------------------ the comparison
def _bits(t):
    """The tensor's bits as integers (bitwise equality implies ``torch.equal``; it also tells -0.0 from 0.0)."""
    if not t.is_floating_point():
        return t
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def state_mismatches(got, want):
    """``[(name, differing elements)]`` over two dicts of tensors; a missing tensor, dtype or shape counts as -1."""
    bad = [(k, -1) for k in sorted(set(got) ^ set(want))]
    for k in sorted(set(got) & set(want)):
        a, b = got[k], want[k]
        if a.dtype != b.dtype or a.shape != b.shape:
            bad.append((k, -1))
        elif not torch.equal(_bits(a), _bits(b)):
            bad.append((k, int((_bits(a) != _bits(b)).sum())))
    return bad


def first_loss_diff(got, want):
    """1-based index of the first step whose losses differ (a missing step differs), or None."""
    for i in range(max(len(got), len(want))):
        if i >= len(got) or i >= len(want) or got[i] != want[i]:
            return i + 1
    return None


def assert_same_run(got_losses, want_losses, got_state, want_state, what):
    step, bad = first_loss_diff(got_losses, want_losses), state_mismatches(got_state, want_state)
    assert step is None and not bad, (
        f"{what}: losses first differ at step {step} (got {got_losses}, want {want_losses}); "
        f"state tensors differing (name, elements): {bad}")


def test_comparison_rejects_one_bit_and_one_loss():
    """Self-check on the CPU: one mantissa bit of one parameter, or the fourth loss, fails the comparison."""
    g = torch.Generator().manual_seed(0)
    want = {"params": torch.randn(257, generator=g), "exp_avg": torch.randn(257, generator=g),
            "mirror": torch.randn(257, generator=g).to(torch.bfloat16), "step_t": torch.tensor([6])}
    losses = [6.9, 6.5, 6.25, 6.0, 5.5, 5.25]
    same = {k: v.clone() for k, v in want.items()}
    assert_same_run(list(losses), losses, same, want, "identical")
    bit = {k: v.clone() for k, v in want.items()}
    bit["params"].view(torch.int32)[100] ^= 1
    assert abs(float(bit["params"][100] - want["params"][100])) < 1e-6
    assert state_mismatches(bit, want) == [("params", 1)]
    with pytest.raises(AssertionError, match=r"\('params', 1\)"):
        assert_same_run(list(losses), losses, bit, want, "one mantissa bit")
    for k, flip in (("mirror", torch.int16), ("step_t", torch.int64)):
        other = {n: v.clone() for n, v in want.items()}
        other[k].view(flip)[0] ^= 1
        assert state_mismatches(other, want) == [(k, 1)]
    zero = {"p": torch.zeros(4)}
    assert state_mismatches({"p": -torch.zeros(4)}, zero) == [("p", 4)]  # bits, not values
    assert state_mismatches({}, zero) == [("p", -1)] and state_mismatches({"p": torch.zeros(5)}, zero) == [("p", -1)]
    fourth = list(losses)
    fourth[3] = float(torch.nextafter(torch.tensor(6.0, dtype=torch.float64), torch.tensor(7.0, dtype=torch.float64)))
    assert first_loss_diff(fourth, losses) == 4 and first_loss_diff(losses[:5], losses) == 6
    with pytest.raises(AssertionError, match="first differ at step 4"):
        assert_same_run(fourth, losses, same, want, "fourth loss")


# ------------------------------------------------------------------------------------------------ single GPU
def _snap(r):
    """What the comparisons need of a finished ``train`` (on the host), then the engine is released."""
    eng = r["engine"]
    eng.check_health()
    torch.cuda.synchronize()
    f, st = eng.flat, eng.stage
    state = {"params": f.params, "exp_avg": f.exp_avg, "exp_avg_sq": f.exp_avg_sq, "step_t": eng.opt.step_t}
    if f.mirror is not None:
        state["mirror"] = f.mirror
    out = dict(history=list(r["history"]), evals=[(s, dict(e)) for s, e in r["evals"]],
               state={k: v.detach().cpu().clone() for k, v in state.items()},
               lr=eng.opt.lr_value(), grad_norm=eng.opt.grad_norm(),
               live=dict(fuse=bool(st._fuse_fwd or st._fuse_bwd), mirror_t=len(f.mirror_t), wg_sq=st.wg_sq is not None,
                         emb_sq=st.emb_sq is not None, emb_prev=st.emb_prev is not None and st._emb_prev_valid,
                         fp8=len(f.mirror_fp8) if st.fp8 else 0, mx=len(f.mirror_mx) if st.mx else 0,
                         defer=bool(eng.defer_opt), graphs=int(eng.program.n_graphs), n_micro=int(eng.n_micro),
                         sched=eng.opt.sched is not None, act=eng.act_dtype, steps_done=int(eng.steps_done)))
    eng.close()
    return out


def _train(cuda, case, out_dir, **run):
    from distributed_training_compare_jax_amd.train.loop import train

    oc = OptimConfig(**dict(OPT, **CASES[case][1]))
    return _snap(train(_tc(case, out_dir, **run), _mc(), oc, DistInfo(0, 1, 0, cuda, "nccl"), quiet=True,
                       write_csv=False))


_RUNS = {}


def _runs(cuda, case):
    """A, B and C of a case, made once (the reference run is shared by the tests that need it and never changed)."""
    if case not in _RUNS:
        env = CASES[case][2]
        assert all(os.environ.get(k) == v for k, v in env.items()), f"{case}: set {env} before the engines are built"
        ck, plan = _tmpdir(), CASES[case][3]
        res = dict(dir=ck)
        res["A"] = _train(cuda, case, _tmpdir(), **plan["A"])
        res["B"] = _train(cuda, case, ck, **plan["B"])
        assert os.path.isfile(os.path.join(ck, "ckpt", f"step_{CKPT}", "rank0.pt"))
        res["C"] = _train(cuda, case, ck, **plan["C"])
        print(f"RESUME {case}: A {res['A']['history']} | C {res['C']['history']} | grad norm after A "
              f"{res['A']['grad_norm']:.4f}, after B {res['B']['grad_norm']:.4f} | lr A {res['A']['lr']:.6g} "
              f"C {res['C']['lr']:.6g}")
        _RUNS[case] = res
    return _RUNS[case]


def _assert_live(case, run, snap):
    """The feature a case is named for ran in the engine under test: a vacuous case fails."""
    live, what = snap["live"], f"{case} run {run}: {snap['live']}"
    if case in ("default", "warmup_offset", "eval"):
        assert live["fuse"] and live["mirror_t"] > 0 and live["wg_sq"] and live["emb_sq"] and live["emb_prev"], what
        assert live["graphs"] >= 1 and live["act"] == torch.bfloat16, what
    if case == "fused_norm_off":
        assert not live["wg_sq"] and not live["emb_sq"] and live["mirror_t"] > 0 and live["fuse"], what
    if case == "eager":
        assert live["graphs"] == 0 and live["wg_sq"], what
    if case == "fp32":
        assert live["act"] == torch.float32 and "mirror" not in snap["state"] and not live["wg_sq"], what
    if case == "fp8":
        assert live["fp8"] == 8 and live["mx"] == 0, what
    if case == "mxfp8":
        assert live["mx"] == 8 and live["fp8"] == 0, what
    if case == "defer_optimizer":
        assert live["defer"] and live["graphs"] >= 1, what
    if case == "accum_schedule":
        assert live["n_micro"] == 2 and live["sched"] and live["wg_sq"], what
    if case == "eval":
        assert snap["evals"] and snap["evals"][-1][1]["tokens"] == 2 * 4 * 128, what


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_bitwise(cuda, monkeypatch, case):
    """B's losses followed by C's are A's, and C ends on A's parameters, Adam state, step counter and bf16 mirror."""
    for k, v in CASES[case][2].items():
        monkeypatch.setenv(k, v)
    runs = _runs(cuda, case)
    a, b, c = runs["A"], runs["B"], runs["C"]
    for run in "ABC":
        _assert_live(case, run, runs[run])
    assert len(c["history"]) == 3 and c["live"]["steps_done"] == 3 and int(c["state"]["step_t"]) == STEPS
    assert_same_run(b["history"] + c["history"], a["history"], c["state"], a["state"], f"{case}: B + C against A")
    if case == "accum_schedule":  # the checkpoint falls mid-schedule: warmup over, the cosine not yet at its floor
        assert c["lr"] == a["lr"] and 0.0 <= a["lr"] < OPT["lr"], (c["lr"], a["lr"])
        assert b["lr"] != a["lr"], (b["lr"], a["lr"])
    else:
        assert c["lr"] == a["lr"] == OPT["lr"]
    if case == "eval":
        (sa, ea), (sc, ec) = a["evals"][-1], c["evals"][-1]
        assert (sa, sc) == (STEPS, STEPS - CKPT) and len(a["evals"]) == 2 and len(c["evals"]) == 1
        assert (ec["loss"], ec["ppl"], ec["top1"], ec["tokens"]) == (ea["loss"], ea["ppl"], ea["top1"], ea["tokens"]), (ec, ea)
        assert b["evals"][-1][1] == a["evals"][0][1], (b["evals"], a["evals"])
        # the evaluation reads the parameters and nothing else: the training run is the default case's
        assert a["history"] == _runs(cuda, "default")["A"]["history"]
        assert not state_mismatches(a["state"], _runs(cuda, "default")["A"]["state"])


@gpu
@pytest.mark.parametrize("case", ["default", "defer_optimizer"])
def test_saving_does_not_disturb_the_run(cuda, case):
    """6 steps with a checkpoint after the third (and the sixth): A's losses and final state; the step-3 files hold
    what B wrote (for ``defer_optimizer`` the save flushes the pending update, and the next replay must not apply
    it again)."""
    runs = _runs(cuda, case)
    td = _tmpdir()
    d = _train(cuda, case, td, warmup_steps=0, steps=STEPS, ckpt_every=CKPT)
    _assert_live(case, "D", d)
    assert_same_run(d["history"], runs["A"]["history"], d["state"], runs["A"]["state"], f"{case}: saving run against A")
    mine, theirs = (torch.load(os.path.join(x, "ckpt", f"step_{CKPT}", "rank0.pt"), map_location="cpu",
                               weights_only=True) for x in (td, runs["dir"]))
    assert mine.pop("step") == theirs.pop("step") == CKPT and int(mine["step_t"]) == CKPT
    assert sorted(mine) == ["exp_avg", "exp_avg_sq", "params", "step_t"]
    assert not state_mismatches(mine, theirs), state_mismatches(mine, theirs)
    last = torch.load(os.path.join(td, "ckpt", f"step_{STEPS}", "rank0.pt"), map_location="cpu", weights_only=True)
    last.pop("step")
    want = {k: runs["A"]["state"][k] for k in last}
    assert not state_mismatches(last, want), state_mismatches(last, want)


@gpu
def test_resume_from_every_step(cuda):
    """The default path resumed after each of steps 1 .. 5 for one step: the loss is A's, and the checkpoint the
    resumed engine writes after that step holds the bits of the straight run's.  (Whether two summation orders of the
    global norm give the same fp32 sum is a matter of the step's data: while a resumed engine still took its first
    norm from the plain pass, the runs resumed after steps 1, 3 and 5 agreed with A and the ones resumed after steps 2
    and 4 differed in 108175 and 39860 parameters.)"""
    a = _runs(cuda, "default")["A"]
    src = _tmpdir()
    d = _train(cuda, "default", src, warmup_steps=0, steps=STEPS, ckpt_every=1)
    assert_same_run(d["history"], a["history"], d["state"], a["state"], "a checkpoint after every step against A")
    load = lambda root, k: torch.load(os.path.join(root, "ckpt", f"step_{k}", "rank0.pt"), map_location="cpu",  # noqa: E731
                                      weights_only=True)
    bad = []
    for k in range(1, STEPS):
        td = _tmpdir()
        shutil.copytree(os.path.join(src, "ckpt", f"step_{k}"), os.path.join(td, "ckpt", f"step_{k}"))
        c = _train(cuda, "default", td, warmup_steps=0, steps=1, resume=True, ckpt_every=1)
        assert c["live"]["fuse"] and c["live"]["wg_sq"] and c["live"]["emb_sq"] and c["live"]["mirror_t"] > 0, c["live"]
        got, want = load(td, k + 1), load(src, k + 1)
        assert got.pop("step") == want.pop("step") == k + 1 and c["live"]["steps_done"] == 1
        diff = state_mismatches(got, want)
        if c["history"] != a["history"][k:k + 1] or diff:
            bad.append((k, c["history"], a["history"][k:k + 1], diff))
        if k == STEPS - 1:  # ... and the bf16 mirror, which no checkpoint holds
            assert_same_run(c["history"], a["history"][k:], c["state"], a["state"], "resumed after step 5")
    assert not bad, f"(resumed after step, loss, A's loss, state tensors differing (name, elements)): {bad}"


@gpu
@pytest.mark.parametrize("case", ["default", "fp8", "mxfp8"])
def test_load_into_rebuilds_what_a_checkpoint_leaves_out(cuda, case):
    """Straight after ``load_into`` on a fresh engine, before any step: the kernels that rebuild the mirrors against
    references computed on the CPU from the checkpoint's parameters."""
    from distributed_training_compare_jax_amd.ops import fp8 as F8
    from distributed_training_compare_jax_amd.ops import mxfp8 as MX
    from distributed_training_compare_jax_amd.train.engine import Engine
    from distributed_training_compare_jax_amd.utils.checkpoint import load_into

    ck_dir = _runs(cuda, case)["dir"]
    oc = OptimConfig(**dict(OPT, **CASES[case][1]))
    eng = Engine(_mc(), _tc(case, ck_dir, warmup_steps=0, steps=3, resume=True), oc, DistInfo(0, 1, 0, cuda, "nccl"))
    f = eng.flat
    init = f.params.cpu().clone()
    assert load_into(eng, ck_dir, CKPT) == CKPT and eng.steps_done == 0
    torch.cuda.synchronize()
    ck = torch.load(os.path.join(ck_dir, "ckpt", f"step_{CKPT}", "rank0.pt"), map_location="cpu", weights_only=True)
    got = {"params": f.params.cpu(), "exp_avg": f.exp_avg.cpu(), "exp_avg_sq": f.exp_avg_sq.cpu(),
           "step_t": eng.opt.step_t.cpu()}
    assert not state_mismatches(got, {k: ck[k] for k in got}) and int(ck["step_t"]) == CKPT
    params, n = got["params"], f.n_mirror
    assert int((params != init).sum()) > n // 2, "the checkpoint holds the initial parameters: nothing to rebuild"
    assert int(f.grads.count_nonzero()) == 0
    # the bf16 mirror: round to nearest even of the fp32 master (torch's CPU conversion)
    want = params[:n].to(torch.bfloat16)
    assert n > 0 and torch.equal(f.mirror[:n].cpu().view(torch.int16), want.view(torch.int16)), \
        int((f.mirror[:n].cpu().view(torch.int16) != want.view(torch.int16)).sum())
    w_cpu = lambda sl: want[sl.offset:sl.offset + sl.numel].view(sl.shape)  # noqa: E731
    assert len(f.mirror_t) == 7, sorted(f.mirror_t)  # fc1, qkv, out of both layers and the lm_head
    for name, (sl, t) in f.mirror_t.items():
        assert tuple(t.shape) == (sl.shape[1], sl.shape[0]) and torch.equal(t.cpu(), w_cpu(sl).t()), name
    assert len(f.mirror_fp8) == (8 if case == "fp8" else 0) and len(f.mirror_mx) == (8 if case == "mxfp8" else 0)
    for name, (sl, t) in f.mirror_fp8.items():
        ref = F8.quant_e4m3(w_cpu(sl).contiguous())  # the torch branch: a CPU tensor
        assert torch.equal(t.q.cpu(), ref.q), (name, int((t.q.cpu() != ref.q).sum()))
        assert torch.equal(_bits(t.scale.cpu()), _bits(ref.scale)) and torch.equal(_bits(t.inv.cpu()), _bits(ref.inv)), name
    for name, (sl, t) in f.mirror_mx.items():
        ref = MX.quant_mxfp8(w_cpu(sl).contiguous())
        assert torch.equal(t.q.cpu(), ref.q), (name, int((t.q.cpu() != ref.q).sum()))
        assert torch.equal(t.sc.cpu(), ref.sc), (name, int((t.sc.cpu() != ref.sc).sum()))
    # the next step is step 4 of the run: its global norm comes from the fused partials, as in the straight run
    st = eng.stage
    assert st.wg_record and st.wg_sq is not None and st.emb_sq is not None
    assert st.emb_prev is not None and not st._emb_prev_valid  # the first embedding backward zeroes the whole table
    eng.close()


@gpu
def test_stage_lists_its_grouped_wgrad_problems(cuda):
    """What a resumed engine registers the Σ dW² partials from (``GPTStage.wgrad_problems``) is what the first step's
    grouped launch records (``wg_seen``): the same gradient tensors, in launch order, with the same shapes."""
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.train.engine import Engine

    mc = _mc()
    eng = Engine(mc, _tc("default", "/tmp/unused", warmup_steps=0, steps=1), OptimConfig(**OPT),
                 DistInfo(0, 1, 0, cuda, "nccl"))
    st = eng.stage
    assert st.wg_record and st.wg_seen is None and st.wg_sq is None
    listed = st.wgrad_problems()
    eng.set_batch(next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    eng.run_step()
    eng.loss_value()
    seen = st.wg_seen
    assert st.wg_sq is not None and seen is not None and len(seen) == len(listed) == 1 + 4 * mc.n_layers
    for (dw, m, n), (dw2, m2, n2) in zip(seen, listed):
        assert dw.data_ptr() == dw2.data_ptr() and tuple(dw.shape) == tuple(dw2.shape) == (m, n) == (m2, n2)
    assert seen[0][0].data_ptr() == eng.flat.g("lm_head.w").data_ptr()
    assert [s[0].data_ptr() for s in seen[1:5]] == [eng.flat.g(f"h.1.{x}.w").data_ptr()
                                                    for x in ("fc2", "fc1", "out", "qkv")]
    eng.close()


# ------------------------------------------------------------------------------------------------ two processes
LAYOUTS = {
    "tp2_sp": ("tp", dict(tp_sequence_parallel=True)),
    "pp2_1f1b": ("pp", dict(pp_schedule="1f1b", pp_microbatches=2, pp_clip="global", pp_head_split=True)),
    "dp2": ("dp", {}),
}


def _worker(parallel, kw, run, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    tc = TrainConfig(seed=0, parallel=parallel, batch=4, log_every=1000, device="cuda", **dict(kw, **run))
    d = init_distributed("cuda")
    r = train(tc, mc, OptimConfig(**OPT), d, quiet=True, write_csv=False)
    eng = r["engine"]
    eng.check_health()
    torch.cuda.synchronize()
    f, m = eng.flat, eng.mesh
    torch.save({"losses": r["history"], "mesh": (m.dp, m.tp, m.pp), "sp": eng.stage.sp,
                "head_part": eng.stage.layout.head_part, "n_micro": eng.n_micro, "dp_comm": eng.dp_comm,
                "p2p": any(t is not None for t in eng._transports.values()),
                "state": {"params": f.params.cpu(), "exp_avg": f.exp_avg.cpu(), "exp_avg_sq": f.exp_avg_sq.cpu(),
                          "step_t": eng.opt.step_t.cpu()}},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


def _spawn2(parallel, kw, run):
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, 2, args=(parallel, kw, run, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(2)]


@gpu
@pytest.mark.slow
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_resume_is_bitwise_two_ranks(cuda, layout):
    """A, B and C with two ranks on one GPU: both ranks read A's losses, and each rank's parameters and Adam state
    after C are its own after A."""
    parallel, kw = LAYOUTS[layout]
    ck = _tmpdir()
    a = _spawn2(parallel, kw, dict(PLAIN["A"], output_dir=_tmpdir()))
    b = _spawn2(parallel, kw, dict(PLAIN["B"], output_dir=ck))
    assert all(os.path.isfile(os.path.join(ck, "ckpt", f"step_{CKPT}", f"rank{r}.pt")) for r in range(2))
    c = _spawn2(parallel, kw, dict(PLAIN["C"], output_dir=ck))
    print(f"RESUME {layout}: A {a[0]['losses']} | C {c[0]['losses']}")
    want = {"tp2_sp": (1, 2, 1), "pp2_1f1b": (1, 1, 2), "dp2": (2, 1, 1)}[layout]
    for r in a + b + c:  # the layout under test ran, on the process-group path
        assert r["mesh"] == want and not r["p2p"], (r["mesh"], r["p2p"])
        assert r["sp"] == (layout == "tp2_sp") and r["dp_comm"] == (layout == "dp2")
        assert r["n_micro"] == (2 if layout == "pp2_1f1b" else 1)
    if layout == "pp2_1f1b":
        assert [r["head_part"] for r in c] == [(0, 2), (1, 2)]
    assert a[0]["losses"] == a[1]["losses"] and len(a[0]["losses"]) == STEPS
    for rank in range(2):
        assert int(c[rank]["state"]["step_t"]) == STEPS
        assert_same_run(b[rank]["losses"] + c[rank]["losses"], a[rank]["losses"], c[rank]["state"], a[rank]["state"],
                        f"{layout} rank {rank}: B + C against A")
