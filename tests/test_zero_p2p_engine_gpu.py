"""``zero_comm: p2p`` through the engine, on the rig of tests/test_dp_p2p_engine_gpu.py: DP replicas as processes on ONE
GPU over gloo, trained through ``spawn`` / ``train`` (tiny preset, 4 layers, vocab 1000, batch 4, 6 steps, warmup 2),
with ``dp_bucket_mb=0.25, dp_tail_mb=0.05`` so that a step has several buckets.

Bitwise cases run with ``grad_clip = 1e9``, which the norm never reaches: ``norm < max_norm`` holds, the clip factor is
exactly ``1.f`` in every AdamW kernel (tests/test_adamw_tr_gpu.py holds those kernels equal to each other), and the
parameters no longer depend on the summation order of the norm.  Every element's reduced gradient is then the same
rank-ordered sum as under ``dp_comm: p2p, zero_stage: 0``, so the parameters are ``torch.equal``; two-term fp32 sums
are exact in any order, so dp2 fp32 also equals ``zero_comm: rccl``.  The clipped cases (``grad_clip`` = half the
step-0 norm of the same layout's ``zero_stage: 0`` run) differ from the replicated optimizer in the norm's summation
order only and are held to the single-process run with the tolerances of ``test_dp4_fp32_matches_single_gpu``: loss
rel / abs 2e-2, relative update error < 0.15, the ``qkv.b`` key-bias rows excluded as there.
"""

import atexit
import functools
import os
import shutil
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

from test_dp_p2p_engine_gpu import BUCKETS, PKG, _key, _model_cfg

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
STEPS = 6
NOCLIP = 1e9
ZP2P = dict(zero_stage=1, zero_comm="p2p")
REPL = dict(dp_comm="p2p", zero_stage=0, dp_embed_gather=False)  # the replicated step on the same rank-ordered sums


def _worker(kw, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    kw = dict(kw)
    lib = kw.pop("kernel_lib", None)
    if lib:  # read when ops._native is first imported (a fresh spawned rank)
        os.environ["DTC_KERNEL_LIB"] = lib
    for k, v in kw.pop("env", ()):  # before the package import, like the library above
        os.environ[k] = v
    clip = kw.pop("grad_clip", 1.0)
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig
    from distributed_training_compare_jax_amd.ops import _native
    from distributed_training_compare_jax_amd.ops.payload import cast_to_bf16
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.engine import Engine
    from distributed_training_compare_jax_amd.train.loop import train

    sumsqs, run_step = [], Engine.run_step

    def run_step_and_keep_the_norm(self):  # a device copy behind every step (warmup included): no host sync
        loss = run_step(self)
        sumsqs.append(self.opt.sumsq.clone())
        return loss

    Engine.run_step = run_step_and_keep_the_norm
    base = dict(seed=0, parallel="dp", batch=4, steps=STEPS, log_every=1000, output_dir="/tmp/unused", device="cuda",
                warmup_steps=2)
    base.update(kw)
    tc = TrainConfig(**base)
    d = init_distributed("cuda")
    out = {}
    try:
        r = train(tc, _model_cfg(), OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=clip), d, quiet=True,
                  write_csv=False)
    except ValueError as e:  # a refused resume: raised on every rank before anything was loaded
        torch.save({"error": str(e)}, os.path.join(out_dir, f"rank{d.rank}.pt"))
        destroy()
        return
    eng = r["engine"]
    eng.check_health()
    f = eng.flat
    if f.use_mirror and f.n_mirror > 0:
        want = torch.empty_like(f.mirror[:f.n_mirror])
        cast_to_bf16(f.params[:f.n_mirror], want)
        out["mirror_ok"] = bool(torch.equal(want.view(torch.int16), f.mirror[:f.n_mirror].view(torch.int16)))
        out["mirror_t_ok"] = all(torch.equal(t, f._view(f.mirror, n).t()) for n, (sl, t) in f.mirror_t.items())
        out["n_mirror_t"] = len(f.mirror_t)
    zp = bool(getattr(eng, "zero_p2p", False))
    out.update({"losses": r["history"], "graphs": r["n_graphs"], "comms": r["n_comms"], "params": f.params.cpu(),
                "lib": _native.LIB_PATH, "p2p": eng.dp_p2p is not None, "zero": bool(eng.zero), "zero_p2p": zp,
                "stream": eng.dp_p2p is not None and eng.dp_p2p._cs is not None, "opt": type(eng.opt).__name__,
                "buckets": len(eng.buckets.buckets), "payload": eng.buckets.payload, "gather": eng.embed_gather,
                "norms": [float(x.item()) ** 0.5 for x in sumsqs], "m_numel": f.exp_avg.numel(), "numel": f.numel,
                "owned": sum(hi - lo for lo, hi in eng.opt.owned) if zp else None,
                "named": {n: f.p(n).detach().float().cpu().clone() for n in f.slots}})
    torch.save(out, os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


@functools.lru_cache(maxsize=None)
def _run(world, kw_items):
    """One spawn at a time; a run shared by two tests is made once."""
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, world, args=(dict(kw_items), td))
        return [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(world)]


def _zero(world, **kw):
    res = _run(world, _key(dict(kw, **ZP2P, **BUCKETS)))
    _assert_zero_p2p_run(res, world)
    return res


def _assert_zero_p2p_run(res, world, what=""):
    """What holds for every ``zero_comm: p2p`` run."""
    print(f"ZERO-P2P {what}: graphs/comms per rank {[(r['graphs'], r['comms']) for r in res]}, "
          f"owned {[r['owned'] for r in res]} of {res[0]['numel']}")
    for r in res:
        assert r["zero"] and r["zero_p2p"] and r["p2p"] and r["opt"] == "P2PShardedAdamW" and not r["gather"]
        assert r["buckets"] >= 3
        assert r["graphs"] == 1 and r["comms"] == 0, (what, r["graphs"], r["comms"])
        assert r["m_numel"] == r["owned"]
        if "mirror_ok" in r:
            assert r["mirror_ok"] and r["mirror_t_ok"] and r["n_mirror_t"] > 0
    assert sum(r["owned"] for r in res) == res[0]["numel"]
    for r in res[1:]:  # replicas identical on every rank
        assert torch.equal(r["params"], res[0]["params"]) and r["losses"] == res[0]["losses"]
    assert len(res[0]["losses"]) == STEPS and all(x == x for x in res[0]["losses"])


def _assert_params_equal(a, b, what):
    for r, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["params"], y["params"]), (what, r, int((x["params"] != y["params"]).sum()))


# ------------------------------------------------------------------------------------------------ bitwise (no clip)

def test_dp2_fp32_equals_rccl_zero(cuda):
    """Two-term fp32 sums are exact in any order: the process-group ZeRO-1 (its gloo branch) gives the same bits."""
    res = _zero(2, grad_clip=NOCLIP)
    ref = _run(2, _key(dict(zero_stage=1, zero_comm="rccl", grad_clip=NOCLIP, **BUCKETS)))
    assert all(r["opt"] == "ShardedAdamW" and r["zero"] and not r["zero_p2p"] and not r["p2p"] for r in ref)
    assert all(r["graphs"] >= 2 for r in ref), [r["graphs"] for r in ref]  # cut at every collective
    for a, b in zip(res, ref):
        assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    _assert_params_equal(res, ref, "rccl")


@pytest.mark.parametrize("world,payload", [(2, "fp32"), (2, "bf16"), (4, "bf16"), (4, "fp32")])
def test_equals_the_replicated_p2p_step_bitwise(cuda, world, payload):
    kw = dict(grad_clip=NOCLIP, **({"dp_grad_dtype": "bf16"} if payload == "bf16" else {}))  # (fp32 is the default)
    res = _zero(world, **kw)
    rep = _run(world, _key(dict(REPL, **kw, **BUCKETS)))
    assert all(r["payload"] == payload for r in res + rep) and res[0]["buckets"] == rep[0]["buckets"]
    assert all(r["opt"] == "FusedAdamW" and r["p2p"] and not r["zero"] for r in rep)
    _assert_params_equal(res, rep, (world, payload))
    for a, b in zip(res, rep):  # the loss sum is the same rank-ordered one-shot call
        assert a["losses"] == b["losses"], (a["losses"], b["losses"])


def test_world1_rehearsal_matches_plain_dp1(cuda):
    res = _run(1, _key(dict(ZP2P, dp_comm_rehearsal=True, grad_clip=NOCLIP, env=(("DTC_WORLD1_PG", "1"),), **BUCKETS)))
    plain = _run(1, _key(dict(grad_clip=NOCLIP)))
    _assert_zero_p2p_run(res, 1, "world 1")
    assert not plain[0]["p2p"] and not plain[0]["zero"]
    assert res[0]["losses"] == plain[0]["losses"], (res[0]["losses"], plain[0]["losses"])
    assert torch.equal(res[0]["params"], plain[0]["params"]), int((res[0]["params"] != plain[0]["params"]).sum())


def test_stream_placement_changes_no_bit(cuda):
    """The race check of the fork: the calls on the forked comm stream (1) and on the main stream (0) give the same
    losses and parameters, bit for bit, in the dp2 bf16 case."""
    kw = dict(dp_grad_dtype="bf16", grad_clip=NOCLIP)
    on = _zero(2, **kw, env=(("DTC_DP_P2P_STREAM", "1"),))
    off = _zero(2, **kw, env=(("DTC_DP_P2P_STREAM", "0"),))
    assert all(r["stream"] for r in on) and not any(r["stream"] for r in off)
    for a, b in zip(on, off):
        assert a["losses"] == b["losses"], (a["losses"], b["losses"])
        assert torch.equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
    dflt = _zero(2, **kw)  # the default is the fork
    assert all(r["stream"] for r in dflt) and torch.equal(dflt[0]["params"], on[0]["params"])


# ------------------------------------------------------------------------------------------------ clipped

@pytest.mark.parametrize("world", [2, 4])
def test_clipped_step_matches_single_gpu(cuda, world):
    from distributed_training_compare_jax_amd.models.params import all_param_specs, init_full

    # the step-0 norm does not depend on the clip: the replicated run of the same layout that the bitwise cases use
    probe = _run(world, _key(dict(REPL, grad_clip=NOCLIP, **BUCKETS)))
    clip = 0.5 * probe[0]["norms"][0]
    assert clip > 0
    res = _zero(world, grad_clip=clip)
    single = _run(1, _key(dict(grad_clip=clip)))
    print(f"ZERO-P2P clipped dp{world}: clip {clip:.4f}, norms {res[0]['norms']}")
    assert len(res[0]["norms"]) == STEPS + 2 and max(res[0]["norms"]) > clip  # the clip branch ran
    assert all(r["norms"] == res[0]["norms"] for r in res)  # every rank holds the same bits of the global norm
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=2e-2, abs=2e-2), (res[0]["losses"],
                                                                                         single[0]["losses"])
    p0 = {sp.name: init_full(sp, 0) for sp in all_param_specs(_model_cfg())}
    full, one = res[0]["named"], single[0]["named"]
    assert set(full) == set(one)
    for n in one:
        a, b, q = full[n], one[n], p0[n]
        if n.endswith("qkv.b"):  # key bias: analytically zero gradient, Adam normalises its noise
            a, b, q = (x.view(3, -1)[[0, 2]] for x in (a, b, q))
        err = (((a - q) - (b - q)).norm() / ((b - q).norm() + 1e-12)).item()
        assert err < 0.15, f"{n}: update differs from the single-GPU run by {err:.3f} (relative)"


# ------------------------------------------------------------------------------------------------ checkpoints

CKPT = dict(ZP2P, grad_clip=NOCLIP, **BUCKETS)


@functools.lru_cache(maxsize=None)
def _checkpoint():
    """dp2, 3 steps (2 of them the warmup) and a checkpoint; made once, its directory kept until the session ends."""
    td = tempfile.mkdtemp()
    atexit.register(shutil.rmtree, td, ignore_errors=True)
    first = _run(2, _key(dict(CKPT, warmup_steps=2, steps=1, ckpt_every=3, output_dir=td)))
    assert all("error" not in r for r in first) and os.path.isdir(os.path.join(td, "ckpt", "step_3"))
    return td


def test_checkpoint_resume_is_bitwise(cuda):
    """3 steps, a checkpoint, a resumed run of 3 more steps = 6 straight steps, ``torch.equal``."""
    straight = _run(2, _key(dict(CKPT, warmup_steps=2, steps=4)))
    second = _run(2, _key(dict(CKPT, warmup_steps=0, steps=3, resume=True, output_dir=_checkpoint())))
    assert all("error" not in r for r in straight + second)
    for a, b in zip(second, straight):
        assert torch.equal(a["params"], b["params"]), int((a["params"] != b["params"]).sum())
        assert a["losses"] == b["losses"][-3:], (a["losses"], b["losses"])
        assert a["m_numel"] == a["owned"] and a["zero_p2p"] and a["graphs"] == 1 and a["comms"] == 0


def test_resume_under_another_transport_raises(cuda):
    """The same checkpoint under ``zero_comm: rccl``: raises on every rank, naming the field, before anything loads."""
    bad = _run(2, _key(dict(CKPT, warmup_steps=0, steps=3, resume=True, output_dir=_checkpoint(), zero_comm="rccl")))
    for r in bad:
        assert "error" in r and "zero_comm" in r["error"], r.get("error")


# ------------------------------------------------------------------------------------------------ debug library

def test_debug_build_runs_the_new_asserts_clean(cuda):
    """One dp2 bf16 case on the -DDTC_DEBUG library (every DTC_ASSERT of the reduce-scatter and gather kernels live),
    selected with DTC_KERNEL_LIB in the spawned ranks as tests/test_dp_p2p_engine_gpu.py does."""
    dbg = os.path.join(PKG, "_dtc_kernels_debug.so")
    assert os.path.exists(dbg), "debug kernel library missing: __graft_entry__.build() builds it in-tree"
    kw = dict(dp_grad_dtype="bf16", grad_clip=NOCLIP)
    res = _zero(2, **kw, kernel_lib=dbg)
    rel = _zero(2, **kw)
    assert all(r["lib"] == dbg for r in res) and all(r["lib"] != dbg for r in rel)
    # -O1 kernels round like the release ones up to the GEMMs' accumulation order
    assert res[0]["losses"] == pytest.approx(rel[0]["losses"], rel=2e-2)
