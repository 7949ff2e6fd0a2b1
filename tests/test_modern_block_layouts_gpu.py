"""The modern block (``pos_emb: rope``, ``norm: rmsnorm``, ``mlp: swiglu``, ``qk_norm: rmsnorm``) on the HIP path under
every layout ``Engine.__init__`` says it runs under.  The kernels have their own float64 tests; this file holds the
Python plumbing around them (docs/NUMERICS.md, "Modern block under layouts"):

1. one real ``run_step`` at ``grad_accum=k`` against the float64 oracle, each parameter held to 2x the k = 1 error of
   the same model and precision (tests/test_grad_accum_gpu.py's method): the ``beta`` of the second and later
   microbatches on ``qn.g`` / ``kn.g``, the RMSNorm gains with their fused ``out.b`` / ``fc2.b``, the SwiGLU ``fc2``;
2. dp, ZeRO-1 (process group and ``zero_comm: p2p``), ``dp_comm: p2p`` and the pipeline schedules (gpipe, 1f1b, zb with
   its B/W split, the split head, ``pp_comm: p2p``) against a single-process run, 2-4 processes on one GPU over gloo
   with tests/test_dist_gpu.py's harness and bounds;
3. checkpoint resume bit for bit (tests/test_resume_gpu.py's A / B / C runs and ``assert_same_run``);
4. the evaluation loss, the document mask and d_model 2048 (the unfused SwiGLU by default, the fused pair under
   ``DTC_SWIGLU_FUSE=2``, with its kernel-level twin at K = 2048) against the oracle.

``qkv.b`` is compared in full everywhere: the rotation and the head norm both break the softmax's shift invariance, so
the key bias's gradient is not zero for these models."""

import functools
import os
import tempfile

import pytest
import torch
from test_attn_doc_engine_gpu import GRAD_TOL as DOC_GRAD_TOL
from test_attn_doc_engine_gpu import LOSS_TOL as DOC_LOSS_TOL
from test_attn_doc_engine_gpu import SEP
from test_attn_doc_engine_gpu import _batches as doc_batches
from test_dist_gpu import _full_params
from test_dist_gpu import _run as dist_run
from test_modern_block_layouts_cpu import (FULL_BF16, FULL_F32, FULL_HD128, MODERN, WATCHED, grad_errors, model, one_step,
                                           oracle, print_watched)
from test_resume_gpu import CKPT, OPT, PLAIN, SCHED, STEPS, _snap, _tmpdir, assert_same_run
from test_resume_gpu import _mc as resume_mc
from test_swiglu_gpu import _run as swiglu_run

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset, replace
from distributed_training_compare_jax_amd.data import synthetic
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import swiglu as SW
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = [pytest.mark.gpu, pytest.mark.slow]  # as tests/test_dist_gpu.py, whose harness part 2 runs on

MODELS = {"FULL_BF16": (FULL_BF16, "bf16"), "FULL_HD128": (FULL_HD128, "bf16"), "FULL_F32": (FULL_F32, "fp32")}


# ---------------------------------------------------------------- 1. the accumulated step against the float64 oracle
@functools.lru_cache(maxsize=None)
def _base(name, batch, kw_items=()):
    """The k = 1 step of this model, precision and batch, its float64 oracle and its errors (computed once, never
    modified)."""
    over, dtype = MODELS[name]
    mc = model(over)
    eng, b, p0, loss, grads = one_step(mc, "cuda:0", 1, batch, dtype=dtype, **dict(kw_items))
    ref_loss, ref_grads = oracle(mc, p0, b)
    return dict(mc=mc, ref_loss=ref_loss, ref_grads=ref_grads, errs=grad_errors(grads, ref_grads),
                lerr=abs(loss - ref_loss), last=dict(SW.LAST))


@pytest.mark.parametrize("name,batch,k,kw", [("FULL_BF16", 8, 2, {}), ("FULL_BF16", 8, 4, {}), ("FULL_F32", 8, 2, {}),
                                             ("FULL_HD128", 8, 2, {}), ("FULL_BF16", 8, 2, dict(wgrad_group=-1))],
                         ids=["bf16_k2", "bf16_k4", "fp32_k2", "hd128_k2", "bf16_k2_wgrad_now"])
def test_accumulated_step_matches_oracle(cuda, name, batch, k, kw):
    """``wgrad_group=-1``: the weight gradients launched one by one with ``GPTStage._beta`` instead of the grouped
    launch that takes ``beta`` as an argument (the base is the k = 1 step under the same setting)."""
    base = _base(name, batch, tuple(kw.items()))
    over, dtype = MODELS[name]
    eng, b, p0, loss, grads = one_step(base["mc"], "cuda:0", k, batch, dtype=dtype, **kw)
    assert eng.stage._defer_wg == (not kw) and eng.stage.qkn and eng.stage.rms and eng.stage.glu
    assert "h.0.qn.g" in grads and "h.1.kn.g" in grads and "wpe" not in grads and "h.0.ln1.b" not in grads
    if name == "FULL_BF16":
        assert SW.LAST == {"fc1": "fused", "fc2_dgrad": "fused"} == base["last"], (SW.LAST, base["last"])
    errs, lerr = grad_errors(grads, base["ref_grads"]), abs(loss - base["ref_loss"])
    what = f"{name} {dtype} batch {batch} k {k} {kw}"
    print_watched(what, errs, base["errs"])
    ratios = {n: errs[n] / base["errs"][n] for n in errs}
    worst = max(ratios, key=ratios.get)
    print(f"MODERN | {what} | grad error / k=1 error in [{min(ratios.values()):.3f}, {ratios[worst]:.3f}] (worst {worst}: "
          f"{errs[worst]:.3e} vs {base['errs'][worst]:.3e}) | loss error {lerr:.3e} vs {base['lerr']:.3e}")
    for n in errs:
        assert errs[n] <= 2.0 * base["errs"][n], f"{what} {n}: {errs[n]:.3e} > 2 x {base['errs'][n]:.3e}"
    # the fp32 loss scalar has a rounding of its own (2^-24 relative) below which no error can be held
    assert lerr <= 2.0 * max(base["lerr"], abs(base["ref_loss"]) * 2.0 ** -24), (lerr, base["lerr"])


def test_accumulated_graph_replay_matches_eager_in_one_graph(cuda):
    """tests/test_grad_accum_gpu.py ``test_graph_replay_matches_eager_in_one_graph`` on ``FULL_BF16``."""
    mc, losses = model(FULL_BF16), {}
    for mode in (False, True):
        tc = TrainConfig(seed=0, parallel="dp", batch=8, steps=5, log_every=1, output_dir="/tmp/x", use_graph=mode,
                         grad_accum=2)
        eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, cuda, "nccl"))
        it, out = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999), []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        losses[mode] = out
        if mode:
            assert eng.program.n_graphs == 1 and eng.program.n_comms == 0, (eng.program.n_graphs, eng.program.n_comms)
            assert int(eng.opt.step_t.item()) == 5 and eng.n_micro == 2
            assert SW.LAST == {"fc1": "fused", "fc2_dgrad": "fused"}, SW.LAST
    assert losses[True] == pytest.approx(losses[False], rel=1e-5, abs=1e-5), losses


# --------------------------------------------------------------------------- 2. layouts against a single-process run
PP = {"pp_clip": "global"}
FP32_LAYOUTS = [
    ("dp", 2, {}),
    ("dp", 2, {"zero_stage": 1}),
    ("dp", 2, {"zero_stage": 1, "zero_comm": "p2p"}),
    ("dp", 2, {"dp_comm": "p2p"}),
    ("pp", 2, dict(PP, pp_microbatches=2)),  # gpipe
    ("pp", 2, dict(PP, pp_microbatches=2, pp_schedule="1f1b")),
    ("pp", 4, dict(PP, pp_microbatches=4, pp_schedule="zb")),  # B/W split: the gain partials and fc2's dW wait in between
    ("pp", 4, dict(PP, pp_microbatches=4, pp_schedule="zb", pp_head_split=True)),
    ("pp", 2, dict(PP, pp_microbatches=2, pp_schedule="1f1b", pp_comm="p2p")),
]
BF16_LAYOUTS = [
    ("dp", 2, {"zero_stage": 1}),
    ("pp", 2, dict(PP, pp_microbatches=2, pp_schedule="zb")),
    ("pp", 4, dict(PP, pp_microbatches=4, pp_schedule="1f1b")),
]


def _lid(case):
    parallel, world, kw = case
    return f"{parallel}{world}" + "".join(f"-{v}" if isinstance(v, str) else f"-{k}{v}" for k, v in kw.items()
                                          if k not in ("pp_clip", "pp_microbatches"))


@functools.lru_cache(maxsize=None)
def _single(name):
    """The single-process run of the 4-layer model (a layer per stage of a 4-stage pipeline), once per precision."""
    over, dtype = MODELS[name]
    return dist_run("dp", 1, model=over, **({"dtype": "fp32"} if dtype == "fp32" else {}))


def _update_errors(res, single, over):
    """Relative difference of the six updates ``p - p0`` of every tensor between the layout and the single-process run
    (tests/test_dist_gpu.py), with ``qkv.b`` in full."""
    from distributed_training_compare_jax_amd.models.params import all_param_specs, init_full

    p0 = {sp.name: init_full(sp, 0) for sp in all_param_specs(model(over, layers=4))}
    full, one = _full_params(res, over), _full_params(single, over)
    assert set(full) == set(one) == set(p0) and "h.3.kn.g" in one and "wpe" not in one and "h.0.ln1.b" not in one
    return {n: (((full[n] - p0[n]) - (one[n] - p0[n])).norm() / ((one[n] - p0[n]).norm() + 1e-12)).item() for n in one}


def _check_layout(name, parallel, world, kw, loss_tol, err_tol):
    over, dtype = MODELS[name]
    single = _single(name)
    res = dist_run(parallel, world, model=over, **dict(kw, **({"dtype": "fp32"} if dtype == "fp32" else {})))
    what = f"{name} {dtype} {parallel}{world} {kw}"
    print(f"MODERN | {what} | losses {res[0]['losses']} | single {single[0]['losses']}")
    errs = _update_errors(res, single, over)
    for n, e in errs.items():
        if n.endswith(WATCHED):
            print(f"MODERN | {what} | {n} | update error {e:.3e}")
    worst = max(errs, key=errs.get)
    print(f"MODERN | {what} | worst update error {worst} {errs[worst]:.3e}")
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=loss_tol, abs=loss_tol), (res[0]["losses"],
                                                                                                single[0]["losses"])
    for n, e in errs.items():
        assert e < err_tol, f"{what} {n}: update differs from the single-GPU run by {e:.3e} (relative)"
    if kw.get("zero_comm") == "p2p" or kw.get("dp_comm") == "p2p" or kw.get("pp_comm") == "p2p":
        assert res[0]["graphs"] == 1 and res[0]["comms"] == 0, (res[0]["graphs"], res[0]["comms"])  # in-graph transport
    else:
        assert res[0]["graphs"] >= 2  # the step was captured and cut at the collectives
    if parallel == "dp":  # replicas stay bit-identical
        assert torch.equal(res[0]["params"], res[1]["params"])


@pytest.mark.parametrize("case", FP32_LAYOUTS, ids=_lid)
def test_fp32_layouts_match_single_gpu(cuda, case):
    """``FULL_F32`` with the exact-fp32 kernels at tests/test_dist_gpu.py ``test_fp32_layouts_match_single_gpu``'s
    bounds: losses 1e-4, per-tensor update error below 1e-3."""
    _check_layout("FULL_F32", *case, 1e-4, 1e-3)


@pytest.mark.parametrize("case", BF16_LAYOUTS, ids=_lid)
def test_bf16_layouts_match_single_gpu(cuda, case):
    """``FULL_BF16`` (GQA) at tests/test_dist_gpu.py ``test_two_ranks_match_single_gpu``'s bounds: losses 2e-2, update
    error below 0.15, DP replicas bit-identical."""
    _check_layout("FULL_BF16", *case, 2e-2, 0.15)


# ------------------------------------------------------------------------------------------ 3. resume, bit for bit
RESUME_MODELS = {"bf16": dict(n_kv_heads=2, **MODERN), "fp32": dict(MODERN)}  # at test_resume_gpu's d_ff 1024, batch 4
RESUME_CASES = {"default": ("bf16", {}, {}), "accum_schedule": ("bf16", dict(grad_accum=2), SCHED),
                "fp32": ("fp32", dict(dtype="fp32"), {})}
RESUME_NAMES = ("h.0.qn.g", "h.1.kn.g")


def _named_state(eng):
    """Every parameter by name and the transposed twin of the bf16 mirror, beside what ``_snap`` keeps of the flat
    buffers."""
    f = eng.flat
    out = {"p." + n: f.p(n).detach().cpu().clone() for n in f.slots}
    out.update({"mirror_t." + n: t.detach().cpu().clone() for n, (_, t) in f.mirror_t.items()})
    return out


def _assert_resume_state(state, bf16):
    assert all("p." + n in state for n in RESUME_NAMES) and "p.wpe" not in state and "p.h.0.ln1.b" not in state
    assert {"params", "exp_avg", "exp_avg_sq", "step_t"} <= set(state)
    if bf16:  # fc1, qkv, out and (for the fused SwiGLU dgrad) fc2 of both layers, and the lm_head
        assert "mirror" in state and "mirror_t.h.0.fc2.w" in state and "mirror_t.h.1.qkv.w" in state, sorted(state)


def _resume_train(cuda, case, out_dir, **run):
    from distributed_training_compare_jax_amd.train.loop import train

    mname, tkw, okw = RESUME_CASES[case]
    tc = TrainConfig(seed=0, parallel="dp", batch=4, log_every=1000, output_dir=out_dir, device="cuda", **dict(tkw, **run))
    r = train(tc, resume_mc(**RESUME_MODELS[mname]), OptimConfig(**dict(OPT, **okw)), DistInfo(0, 1, 0, cuda, "nccl"),
              quiet=True, write_csv=False)
    torch.cuda.synchronize()
    named = _named_state(r["engine"])
    snap = _snap(r)
    snap["state"].update(named)
    return snap


@pytest.mark.parametrize("case", list(RESUME_CASES))
def test_resume_is_bitwise(cuda, case):
    """B's losses followed by C's are A's, and C ends on A's parameters (flat and by name), Adam state, step counter,
    bf16 mirror and its transposed twin, which the load rebuilds."""
    ck = _tmpdir()
    a = _resume_train(cuda, case, _tmpdir(), **PLAIN["A"])
    b = _resume_train(cuda, case, ck, **PLAIN["B"])
    assert os.path.isfile(os.path.join(ck, "ckpt", f"step_{CKPT}", "rank0.pt"))
    c = _resume_train(cuda, case, ck, **PLAIN["C"])
    print(f"MODERN | resume {case}: A {a['history']} | C {c['history']} | grad norm after A {a['grad_norm']:.4f}")
    for s in (a, b, c):
        _assert_resume_state(s["state"], case != "fp32")
        assert s["live"]["n_micro"] == (2 if case == "accum_schedule" else 1)
        assert s["live"]["sched"] == (case == "accum_schedule") and s["live"]["graphs"] >= 1
        assert s["live"]["act"] == (torch.float32 if case == "fp32" else torch.bfloat16)
    assert len(c["history"]) == 3 and c["live"]["steps_done"] == 3 and int(c["state"]["step_t"]) == STEPS
    assert_same_run(b["history"] + c["history"], a["history"], c["state"], a["state"], f"{case}: B + C against A")
    assert c["lr"] == a["lr"] and (case == "accum_schedule") == (b["lr"] != a["lr"]), (a["lr"], b["lr"], c["lr"])


def _resume_worker(run, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    tc = TrainConfig(seed=0, parallel="pp", batch=4, log_every=1000, device="cuda", pp_schedule="1f1b", pp_microbatches=2,
                     pp_clip="global", **run)
    d = init_distributed("cuda")
    r = train(tc, model(FULL_BF16, layers=4), OptimConfig(**OPT), d, quiet=True, write_csv=False)
    eng = r["engine"]
    eng.check_health()
    torch.cuda.synchronize()
    f, m = eng.flat, eng.mesh
    state = {"params": f.params.cpu(), "exp_avg": f.exp_avg.cpu(), "exp_avg_sq": f.exp_avg_sq.cpu(),
             "step_t": eng.opt.step_t.cpu()}
    if f.mirror is not None:
        state["mirror"] = f.mirror.cpu()
    state.update(_named_state(eng))
    torch.save({"losses": r["history"], "mesh": (m.dp, m.tp, m.pp), "n_micro": eng.n_micro, "state": state},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


def _resume_spawn2(run):
    with tempfile.TemporaryDirectory() as td:
        spawn(_resume_worker, 2, args=(run, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(2)]


def test_resume_is_bitwise_pp2_1f1b(cuda):
    """A, B and C with two pipeline stages of two ``FULL_BF16`` layers on one GPU: both ranks read A's losses, and each
    stage's parameters, Adam state and mirrors after C are its own after A."""
    ck = _tmpdir()
    a = _resume_spawn2(dict(PLAIN["A"], output_dir=_tmpdir()))
    b = _resume_spawn2(dict(PLAIN["B"], output_dir=ck))
    assert all(os.path.isfile(os.path.join(ck, "ckpt", f"step_{CKPT}", f"rank{r}.pt")) for r in range(2))
    c = _resume_spawn2(dict(PLAIN["C"], output_dir=ck))
    print(f"MODERN | resume pp2_1f1b: A {a[0]['losses']} | C {c[0]['losses']}")
    assert all(r["mesh"] == (1, 1, 2) and r["n_micro"] == 2 for r in a + b + c)
    assert a[0]["losses"] == a[1]["losses"] and len(a[0]["losses"]) == STEPS
    assert "p.h.0.qn.g" in c[0]["state"] and "p.h.3.kn.g" in c[1]["state"] and "mirror_t.h.2.fc2.w" in c[1]["state"]
    assert not any(n in s["state"] for s in c for n in ("p.wpe", "p.h.0.ln1.b", "p.h.2.ln1.b"))
    for rank in range(2):
        assert int(c[rank]["state"]["step_t"]) == STEPS
        assert_same_run(b[rank]["losses"] + c[rank]["losses"], a[rank]["losses"], c[rank]["state"], a[rank]["state"],
                        f"pp2 1f1b rank {rank}: B + C against A")


# ------------------------------------------------------------------------- 4. evaluation, document mask, width
def _engine(cuda, mc, batch, use_graph=False, **kw):
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=5, log_every=1, output_dir="/tmp/x", use_graph=use_graph, **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, cuda, "nccl"))


# loss tolerances of the engine-against-oracle tests (tests/test_qknorm_engine_gpu.py, tests/test_engine_wide_gpu.py)
@pytest.mark.parametrize("name,loss_tol", [("FULL_BF16", 2e-2), ("FULL_F32", 1e-4)])
def test_evaluation_matches_oracle_and_leaves_training_alone(cuda, name, loss_tol):
    """tests/test_eval_engine_gpu.py's pattern.  After one training step: the evaluation loss over two held-out batches
    against the float64 oracle (dropout 0) on the same rows and parameters.  Then two graph-replayed runs of three
    steps, one with an evaluation after each of the first two: the same loss bits and parameters, so nothing was left
    in ``ctx`` and no saved ``qk_raw`` was reused."""
    over, dtype = MODELS[name]
    mc, B, n_eval = model(over), 8, 2
    dkw = {"dtype": "fp32"} if dtype == "fp32" else {}
    eng = _engine(cuda, mc, B, **dkw)
    it = get_batch_iterator(B, mc.max_seq_len + 1, vocab=999)
    eng.set_batch(next(it))
    eng.run_step()
    eng.loss_value()
    out = eng.evaluate(n_eval)
    p = {n: eng.flat.p(n).detach().double().cpu() for n in eng.flat.slots}
    stream, ref = synthetic.SyntheticTokenStream(vocab=999, seed=0), 0.0
    with torch.no_grad():
        for i in range(n_eval):
            rows = synthetic.heldout_rows(stream, i, 0, B, B, mc.max_seq_len + 1)
            ref += oracle_loss(replace(mc, dropout=0.0), p, torch.from_numpy(rows[:, :-1]).contiguous(),
                               torch.from_numpy(rows[:, 1:]).contiguous(), 0, 0).item() / n_eval
    print(f"MODERN | eval {name}: loss {out['loss']:.6f} oracle {ref:.6f}")
    assert out["tokens"] == n_eval * B * mc.max_seq_len and abs(out["loss"] - ref) < loss_tol, (out, ref)

    def run(evaluate):
        e = _engine(cuda, mc, B, use_graph=True, **dkw)
        bi, losses = get_batch_iterator(B, mc.max_seq_len + 1, vocab=999), []
        for s in range(3):
            e.set_batch(next(bi))
            e.run_step()
            losses.append(e.loss_value())
            if evaluate and s < 2:
                e.evaluate(n_eval)
        torch.cuda.synchronize()
        return losses, e.flat.params.clone(), e.flat.exp_avg_sq.clone()

    (l0, p0, v0), (l1, p1, v1) = run(False), run(True)
    assert l1 == l0 and torch.equal(p1, p0) and torch.equal(v1, v0), (l1, l0)


@pytest.mark.parametrize("heads", [4, 2], ids=["hd64", "hd128"])
def test_document_mask_step_matches_masked_oracle(cuda, heads):
    """MHA with a separator that occurs in the batch (about every 7th token), one real ``run_step``: the loss and every
    gradient against the masked float64 oracle at tests/test_attn_doc_engine_gpu.py's tolerances, and further than
    that from the unmasked oracle."""
    mc = model(dict(FULL_F32, n_heads=heads))
    b = doc_batches(mc, 1, rows=4)[0]
    eng, b, p0, loss, grads = one_step(mc, "cuda:0", 1, 4, b=b, doc_mask_token=SEP)
    assert eng.doc_token == SEP and int((b[:, :-1] == SEP).sum()) > 4 * 8
    ref_loss, ref_grads = oracle(mc, p0, b, doc_mask_token=SEP)
    plain, _ = oracle(mc, p0, b)
    errs = grad_errors(grads, ref_grads)
    worst = max(errs, key=errs.get)
    print(f"MODERN | doc mask head_dim {mc.head_dim}: loss {loss:.6f} masked oracle {ref_loss:.6f} unmasked {plain:.6f}; "
          f"worst relative grad error {worst} {errs[worst]:.3e}")
    assert abs(plain - ref_loss) > 3 * DOC_LOSS_TOL, "the two oracles are too close for this test to tell them apart"
    assert abs(loss - ref_loss) < DOC_LOSS_TOL and abs(loss - plain) > DOC_LOSS_TOL, (loss, ref_loss, plain)
    for n, e in errs.items():
        assert e < DOC_GRAD_TOL, f"{n}: relative grad error {e:.3e}"


def test_document_mask_with_gqa_is_refused(cuda):
    with pytest.raises(ValueError, match=r"n_kv_heads=2 cannot be combined with doc_mask_token=7 \(there are no "
                                         r"document-masked GQA kernels\)"):
        _engine(cuda, model(FULL_BF16), 4, doc_mask_token=SEP)


WIDE_BATCH = 2


def _wide_mc():
    mc = model_config_from_preset("gpt-1.3b", vocab_size=1000, n_layers=2, d_ff=4096, max_seq_len=192, n_kv_heads=4, **MODERN)
    assert mc.d_model == 2048 and mc.head_dim == 128 and (mc.n_heads, mc.kv_heads) == (16, 4)
    return mc


@functools.lru_cache(maxsize=None)
def _wide_oracle():
    """The fp32 autograd oracle of tests/test_engine_wide_gpu.py on the canonical initial parameters with moved gains
    (the same under both knob settings), computed once."""
    from test_qknorm_cpu import _move_gains

    mc = _wide_mc()
    eng = _engine(torch.device("cuda", 0), mc, WIDE_BATCH)
    _move_gains(eng, mc)
    params = {n: eng.flat.p(n).detach().float().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    b = next(get_batch_iterator(WIDE_BATCH, mc.max_seq_len + 1, vocab=999))
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous(), 0, 0)
    lo.backward()
    return lo.item(), {n: t.grad for n, t in params.items()}, {n: t.detach() for n, t in params.items()}


@pytest.mark.parametrize("knob,want", [(None, "unfused"), ("2", "fused")], ids=["default_unfused", "fuse2_fused"])
def test_wide_step_matches_oracle(cuda, monkeypatch, knob, want):
    """d_model 2048, 16 heads of 128 on 4 K/V heads, d_ff 4096, T 192, two layers: one real ``run_step`` against the
    oracle at tests/test_engine_wide_gpu.py's bf16 tolerances.  By default the SwiGLU is unfused there (``FUSE_MAX_K``),
    the RMSNorm backward is the 3-chunk wide one; ``DTC_SWIGLU_FUSE=2`` takes the fused pair at K = 2048."""
    if knob is None:
        monkeypatch.delenv("DTC_SWIGLU_FUSE", raising=False)
    else:
        monkeypatch.setenv("DTC_SWIGLU_FUSE", knob)
    mc = _wide_mc()
    ref_loss, ref_grads, ref_p0 = _wide_oracle()
    eng, b, p0, loss, grads = one_step(mc, "cuda:0", 1, WIDE_BATCH)
    assert eng.act_dtype == torch.bfloat16 and all(torch.equal(p0[n], ref_p0[n]) for n in p0)
    assert SW.LAST == {"fc1": want, "fc2_dgrad": want}, SW.LAST
    errs = grad_errors(grads, ref_grads)
    print_watched(f"wide d2048 bf16 swiglu {want}", errs)
    worst = max(errs, key=errs.get)
    print(f"MODERN | wide d2048 swiglu {want}: loss {loss:.6f} oracle {ref_loss:.6f}; worst {worst} {errs[worst]:.3e}")
    assert abs(loss - ref_loss) < 2e-2, (loss, ref_loss)
    for n, e in errs.items():
        assert e < 5e-2, f"{n}: relative grad error {e:.3e}"


def test_fused_swiglu_pair_at_k2048_vs_float64(cuda, monkeypatch):
    """The kernel-level twin: the fused pair at a k-loop of 32 steps (D = 2048, reached only under ``DTC_SWIGLU_FUSE=2``),
    ragged rows, two hidden tiles, within tests/test_swiglu_gpu.py's ``T(K)``-derived bounds."""
    monkeypatch.setenv("DTC_SWIGLU_FUSE", "2")
    swiglu_run(130, 2048, 128, "fused", "fused K2048")
