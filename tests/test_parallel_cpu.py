"""Multi-process CPU (gloo) tests of every parallel layout against the single-process run.

Each case spawns ``world`` ranks running the real Engine (same code path as the GPUs, with
the CPU reference ops) and compares per-step losses and the final parameters with a
world-size-1 run of the same global batch.  Canonical init + layout-invariant data and
dropout make the comparison exact up to fp32 reduction order.
"""

import os
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.parallel.dist import spawn

STEPS = 4


def _cfgs(parallel, model=None, eps=1e-8, batch=4, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, **dict({"n_layers": 4}, **(model or {})))
    tc = TrainConfig(seed=0, parallel=parallel, batch=batch, steps=STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cpu", warmup_steps=0, **kw)
    oc = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0, eps=eps)
    return mc, tc, oc


def _worker(parallel, kw, out_dir):
    from distributed_training_compare_jax_amd.models.params import unshard
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    torch.set_num_threads(1)
    mc, tc, oc = _cfgs(parallel, **kw)
    d = init_distributed("cpu")
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
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


def _full_params(results, model=None):
    """Reassemble full params from tp shards / pp stages (dp replica 0)."""
    from distributed_training_compare_jax_amd.models.params import all_param_specs, unshard

    mc, _, _ = _cfgs("dp", model=model)
    specs = {s.name: s for s in all_param_specs(mc)}
    pieces = {}
    for r in results:
        if r["dp_idx"] != 0:
            continue
        for n, t in r["params"].items():
            # lm_head of a head split over two pipeline stages: (vocab part, tp shard)
            part = r.get("head_part", (0, 1))[0] if n.startswith("lm_head") else 0
            pieces.setdefault(n, {})[(part, r["tp_idx"])] = t
    out = {}
    for n, p in pieces.items():
        parts = sorted({k[0] for k in p})
        out[n] = torch.cat([unshard(specs[n], [p[k] for k in sorted(p) if k[0] == v]) for v in parts], 0)
    return out


@pytest.fixture(scope="module")
def single():
    return _run("dp", 1)


@pytest.mark.slow
@pytest.mark.parametrize("parallel,world,kw", [
    ("dp", 2, {}),
    ("dp", 2, {"zero_stage": 1}),
    ("dp", 4, {"zero_stage": 1}),
    ("tp", 2, {"tp_sequence_parallel": False}),
    ("pp", 2, {"pp_microbatches": 2, "pp_clip": "global"}),
    ("pp", 2, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "1f1b"}),
    ("dp", 4, {"tp": 2}),
    ("pp", 4, {"dp": 2, "pp_microbatches": 2, "pp_clip": "global"}),
    ("pp", 4, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "1f1b"}),
    ("pp", 4, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "gpipe"}),
    ("pp", 2, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "zb"}),
    ("pp", 4, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "zb"}),
    ("tp", 2, {"tp_sequence_parallel": True}),
    ("dp", 4, {"tp": 2, "tp_sequence_parallel": True}),
    # lm_head + CE split by vocab over the last two pipeline stages
    ("pp", 2, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "1f1b", "pp_head_split": True}),
    ("pp", 4, {"pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "zb", "pp_head_split": True}),
    ("pp", 4, {"dp": 2, "pp_microbatches": 2, "pp_clip": "global", "pp_schedule": "1f1b", "pp_head_split": True}),
    ("tp", 2, {"tp_sequence_parallel": True, "wgrad_group": -1}),
])
def test_layout_matches_single_process(single, parallel, world, kw):
    res = _run(parallel, world, **kw)
    assert "tp_sequence_parallel" not in kw or all(r["sp"] == kw["tp_sequence_parallel"] for r in res)
    ref_losses = single[0]["losses"]
    assert res[0]["losses"] == pytest.approx(ref_losses, rel=1e-4, abs=1e-4)
    full = _full_params(res)
    ref = single[0]["params"]
    assert set(full) == set(ref)
    for n in ref:
        a, b = full[n], ref[n]
        if n.endswith("qkv.b"):
            # the key bias has an analytically-zero gradient (softmax shift invariance); Adam
            # normalises its rounding noise to ±lr per step, so only q and v thirds are compared
            a, b = a.view(3, -1)[[0, 2]], b.view(3, -1)[[0, 2]]
        assert torch.allclose(a, b, rtol=1e-3, atol=2e-5), n


@pytest.mark.slow
def test_pp_local_clip_is_reference_semantics(single):
    """pp_clip=local clips per stage (reference create_train_step.py:190): close, not identical."""
    res = _run("pp", 2, pp_microbatches=2, pp_clip="local")
    assert res[0]["losses"][0] == pytest.approx(single[0]["losses"][0], rel=1e-5)
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=2e-2)


@pytest.mark.slow
def test_zero1_replicas_identical():
    """ZeRO-1: after the all-gather every DP replica holds the same params (bit-identical)."""
    res = _run("dp", 2, zero_stage=1)
    for n in res[0]["params"]:
        assert torch.equal(res[0]["params"][n], res[1]["params"][n]), n


# 12 heads (GPT-2 small's count) on 8 TP ranks: whole heads 2,2,2,2,1,1,1,1 (models/params.py head_split)
HEADS12 = {"d_model": 96, "n_heads": 12, "d_ff": 256, "n_layers": 2}


# the newer model options together (grouped-query attention, rotary positions, RMSNorm, SwiGLU) under tensor
# parallelism: whole groups per rank (2 K/V heads on 2 ranks), the gated fc1's two slabs split by rank
GQA_ROPE_RMS_GLU = {"d_model": 64, "n_heads": 4, "n_kv_heads": 2, "d_ff": 192, "n_layers": 2, "norm": "rmsnorm",
                    "mlp": "swiglu", "pos_emb": "rope"}


@pytest.mark.slow
@pytest.mark.parametrize("parallel,world,kw,model", [
    pytest.param("tp", 8, {}, HEADS12, id="tp-8-kw0"),
    pytest.param("dp", 8, {"tp": 4}, HEADS12, id="dp-8-kw1"),  # dp2 x tp4: 3 heads per rank
    # one sequence of the residual stream per rank
    pytest.param("tp", 8, {"tp_sequence_parallel": True, "batch": 8}, HEADS12, id="tp-8-kw2"),
    pytest.param("tp", 2, {"tp_sequence_parallel": True}, GQA_ROPE_RMS_GLU, id="tp-2-sp-gqa_rope_rms_glu"),
    pytest.param("tp", 2, {"tp_sequence_parallel": False}, GQA_ROPE_RMS_GLU, id="tp-2-gqa_rope_rms_glu"),
])
def test_uneven_heads_match_single_process(parallel, world, kw, model):
    """BASELINE.json config 3 (GPT-2 small at TP=8) needs 12 heads on 8 ranks: losses and the reassembled
    params of the uneven head split match the single-process run.  Adam eps 1e-4 (instead of 1e-8) keeps
    the update linear in near-zero gradients, so fp32 reduction-order noise is not amplified to +-lr
    and the params can be compared at fp32 rounding level (measured max |diff| ~1.3e-7)."""
    kw = dict(kw, model=model, eps=1e-4)
    single = _run("dp", 1, model=model, eps=1e-4, batch=kw.get("batch", 4))
    res = _run(parallel, world, **kw)
    assert "tp_sequence_parallel" not in kw or all(r["sp"] == kw["tp_sequence_parallel"] for r in res)
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=1e-5, abs=1e-5)
    full = _full_params(res, model=model)
    ref = single[0]["params"]
    assert set(full) == set(ref)
    for n in ref:
        assert torch.allclose(full[n], ref[n], rtol=1e-5, atol=1e-6), n


@pytest.mark.slow
@pytest.mark.parametrize("parallel,world,kw", [
    ("dp", 2, {"dp_grad_dtype": "bf16"}),
    ("dp", 4, {"dp_grad_dtype": "bf16"}),
    ("dp", 4, {"dp_grad_dtype": "bf16", "tp": 2}),
    ("tp", 2, {"tp_comm_dtype": "bf16"}),
    ("dp", 4, {"tp": 2, "tp_comm_dtype": "bf16", "dp_grad_dtype": "bf16"}),
    ("pp", 2, {"pp_comm_dtype": "bf16", "pp_microbatches": 2, "pp_clip": "global"}),
    ("pp", 4, {"pp_comm_dtype": "bf16", "pp_microbatches": 4, "pp_clip": "global", "pp_schedule": "1f1b"}),
])
def test_bf16_payloads_match_single_process(parallel, world, kw):
    """bf16 DP gradient buckets (all-to-all + fp32 shard sums + all-gather) and bf16 PP stage messages:
    the step stays within bf16 rounding of the fp32 single-process run (losses 1e-3; Adam eps 1e-4 keeps
    the update linear in the rounding so the params are comparable)."""
    single = _run("dp", 1, eps=1e-4)
    res = _run(parallel, world, eps=1e-4, **kw)
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=1e-3, abs=1e-3)
    from distributed_training_compare_jax_amd.models.params import all_param_specs, init_full

    mc, _, _ = _cfgs("dp")
    p0 = {sp.name: init_full(sp, 0) for sp in all_param_specs(mc)}
    full = _full_params(res)
    ref = single[0]["params"]
    for n in ref:
        # relative difference of the parameter UPDATES (bf16 rounding of a cancelling cross-rank sum can move
        # single elements by a good fraction of lr; the update as a whole must stay within ~1 %)
        du, dr = full[n] - p0[n], ref[n] - p0[n]
        err = ((du - dr).norm() / (dr.norm() + 1e-12)).item()
        assert err < 2e-2, (n, err)
    if parallel == "dp" and "tp" not in kw:  # every replica ends with the same params
        for r in res[1:]:
            for n in ref:
                assert torch.equal(r["params"][n], res[0]["params"][n]), n


def _rehearsal_worker(kw, out_dir):
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    torch.set_num_threads(1)
    mc, tc, oc = _cfgs("dp", dp_comm_rehearsal=True, **kw)
    d = init_distributed("cpu", single_rank_pg=True)  # a ONE-rank gloo group
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
    torch.save({"losses": r["history"], "params": {n: eng.flat.p(n).clone() for n in eng.flat.slots},
                "dp_comm": eng.dp_comm, "zero": eng.zero, "gather": eng.embed_gather},
               os.path.join(out_dir, "rank0.pt"))
    destroy()


@pytest.mark.slow
@pytest.mark.parametrize("kw", [{}, {"dp_embed_gather": False}, {"zero_stage": 1}, {"dp_grad_dtype": "bf16"}])
def test_dp_comm_rehearsal_on_one_rank_group(single, kw):
    """dp_comm_rehearsal: the DP code path (buckets, embedding gather, ZeRO-1, bf16 payload chain) on a
    one-member group is the dp1 math (every collective an identity; bf16 payload: grads rounded once)."""
    with tempfile.TemporaryDirectory() as td:
        spawn(_rehearsal_worker, 1, args=(kw, td))
        r = torch.load(os.path.join(td, "rank0.pt"), weights_only=False)
    assert r["dp_comm"] and r["zero"] == (kw.get("zero_stage") == 1)
    if not r["zero"]:  # (ZeRO-1 reduce-scatters every grad: no embedding gather)
        assert r["gather"] == kw.get("dp_embed_gather", True)
    tol = 2e-2 if kw.get("dp_grad_dtype") == "bf16" else 1e-5
    assert r["losses"] == pytest.approx(single[0]["losses"], rel=tol, abs=tol)


# BASELINE.json's three 8-GPU layouts at world 8 (gloo), on a 12-layer / 12-head model so the layer split,
# the head split and the uneven TP head split are the ones GPT-2 small gets on the node
BASE8 = {"d_model": 96, "n_heads": 12, "d_ff": 256, "n_layers": 12}


@pytest.mark.slow
@pytest.mark.parametrize("parallel,world,kw,fp32", [
    ("dp", 8, {}, True),  # config 2: pure dp8, embedding-output gather (one sequence per rank)
    ("dp", 8, {"dp_grad_dtype": "bf16"}, False),  # config 2 with the bf16 payload chain
    # config 4: pp8, zero-bubble schedule + lm_head/CE split over the last two stages, M = 8
    ("pp", 8, {"pp_microbatches": 8, "pp_clip": "global", "pp_schedule": "zb", "pp_head_split": True}, True),
    ("dp", 8, {"tp": 2, "tp_sequence_parallel": True}, True),  # config 5's mesh: dp4 x tp2 with SP
])
def test_baseline_8gpu_layouts_match_single_process(parallel, world, kw, fp32):
    kw = dict(kw, model=BASE8, eps=1e-4, batch=8)
    single = _run("dp", 1, model=BASE8, eps=1e-4, batch=8)
    res = _run(parallel, world, **kw)
    if parallel == "dp" and "tp" not in kw:
        assert res[0]["mesh"] == (8, 1, 1)
    if parallel == "pp":
        assert res[0]["mesh"] == (1, 1, 8) and res[-1]["head_part"] == (1, 2) and res[-2]["head_part"] == (0, 2)
    if "tp_sequence_parallel" in kw:
        assert res[0]["mesh"] == (4, 2, 1) and all(r["sp"] for r in res)
    tol = 1e-4 if fp32 else 1e-3
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=tol, abs=tol)
    full = _full_params(res, model=BASE8)
    ref = single[0]["params"]
    assert set(full) == set(ref)
    for n in ref:
        a, b = full[n], ref[n]
        if fp32:
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), (n, (a - b).abs().max().item())
        else:
            assert ((a - b).norm() / b.norm()).item() < 2e-3, n
    if parallel == "dp" and "tp" not in kw:  # every replica ends with the same params
        for r in res[1:]:
            for n in ref:
                assert torch.equal(r["params"][n], res[0]["params"][n]), n
