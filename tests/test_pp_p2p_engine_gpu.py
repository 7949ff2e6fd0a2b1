"""``pp_comm: p2p`` through the engine: pipeline stages as processes on ONE GPU over gloo, trained through the same
``spawn`` / ``train`` path as tests/test_dist_gpu.py (tiny preset, 4 layers, vocab 1000, batch 4, 6 steps, warmup 2).

The in-graph transport delivers the same bytes as the process-group path and every kernel is deterministic, so a
layout run with ``pp_comm: p2p`` and again with ``rccl`` (here gloo, host-staged) must give EQUAL loss histories and
``torch.equal`` parameters on every rank: no tolerance.  The loss sum adds zeros (exact in any order); the
``pp_clip: global`` norm sum has two terms at S = 2 (exact either way), while at S = 4 gloo's order is not the
rank order of the in-graph sum, so that case is held to the single-process run with the tolerances
``test_two_ranks_match_single_gpu`` uses.  With dp == 1 the p2p step is ONE hipGraph with no eager collective; the
rccl run of the same case is cut (``graphs >= 2``).
"""

import functools
import os
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
STEPS = 6
PKG = os.path.dirname(os.path.abspath(__import__("distributed_training_compare_jax_amd").__file__))


def _model_cfg():
    from distributed_training_compare_jax_amd.config.schema import model_config_from_preset

    return model_config_from_preset("tiny", vocab_size=1000, n_layers=4)


def _worker(parallel, kw, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    kw = dict(kw)
    lib = kw.pop("kernel_lib", None)
    if lib:  # read when ops._native is first imported (a fresh spawned rank)
        os.environ["DTC_KERNEL_LIB"] = lib
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig
    from distributed_training_compare_jax_amd.ops import _native
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    tc = TrainConfig(seed=0, parallel=parallel, batch=4, steps=STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cuda", warmup_steps=2, **kw)
    d = init_distributed("cuda")
    r = train(tc, _model_cfg(), OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0), d, quiet=True, write_csv=False)
    eng = r["engine"]
    eng.check_health()
    torch.save({"losses": r["history"], "graphs": r["n_graphs"], "comms": r["n_comms"],
                "params": eng.flat.params.cpu(), "lib": _native.LIB_PATH,
                "pipe": eng.pp_pipe is not None, "head_part": eng.stage.layout.head_part,
                "head_split": eng.pp_head_split, "pp_bf16": getattr(eng, "pp_bf16", None),
                "named": {n: eng.flat.p(n).detach().float().cpu().clone() for n in eng.flat.slots},
                "dp_idx": eng.mesh.dp_idx, "pp_idx": eng.mesh.pp_idx},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


@functools.lru_cache(maxsize=None)
def _run(parallel, world, kw_items):
    """One spawn at a time; a run shared by two tests is made once."""
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, world, args=(parallel, dict(kw_items), td))
        return [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(world)]


def _pair(world, kw):
    p2p = _run("pp", world, tuple(sorted(dict(kw, pp_comm="p2p").items())))
    ref = _run("pp", world, tuple(sorted(dict(kw, pp_comm="rccl").items())))
    assert all(r["pipe"] for r in p2p) and not any(r["pipe"] for r in ref)
    return p2p, ref


def _assert_bitwise(p2p, ref, what):
    for r, (a, b) in enumerate(zip(p2p, ref)):
        assert a["losses"] == b["losses"], (what, r, a["losses"], b["losses"])
        assert len(a["losses"]) == STEPS and all(x == x for x in a["losses"])
        assert torch.equal(a["params"], b["params"]), (what, r, int((a["params"] != b["params"]).sum()))
    assert all(r["losses"] == p2p[0]["losses"] for r in p2p)  # every stage holds the summed loss


def _assert_one_graph(p2p, ref, what):
    for r in p2p:  # every message, the loss sum (and the norm sum) in-graph: nothing left between segments
        assert r["graphs"] == 1 and r["comms"] == 0, (what, r["pp_idx"], r["graphs"], r["comms"])
    for r in ref:
        assert r["graphs"] >= 2, (what, r["pp_idx"], r["graphs"])
    print(f"PP-P2P {what}: p2p graphs/comms per stage {[(r['graphs'], r['comms']) for r in p2p]}, "
          f"rccl {[(r['graphs'], r['comms']) for r in ref]}")


LAYOUTS = [
    (2, {"pp_microbatches": 2, "pp_schedule": "gpipe"}),
    (2, {"pp_microbatches": 2, "pp_schedule": "1f1b"}),
    (4, {"pp_microbatches": 4, "pp_schedule": "1f1b"}),
    (4, {"pp_microbatches": 4, "pp_schedule": "zb"}),
    (4, {"pp_microbatches": 4, "pp_schedule": "zb", "pp_head_split": True}),
    (2, {"pp_microbatches": 2, "pp_schedule": "gpipe", "pp_comm_dtype": "fp32"}),
    (2, {"pp_microbatches": 2, "pp_schedule": "1f1b", "pp_clip": "global"}),  # two-term norm sum: exact
]


@pytest.mark.parametrize("world,kw", LAYOUTS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(
    v, dict) else f"pp{v}")
def test_p2p_matches_rccl_bitwise_in_one_graph(cuda, world, kw):
    p2p, ref = _pair(world, kw)
    assert all(r["pp_bf16"] == (kw.get("pp_comm_dtype") != "fp32") for r in p2p)
    assert all(r["head_split"] == bool(kw.get("pp_head_split", r["head_split"])) for r in p2p)
    _assert_bitwise(p2p, ref, kw)
    _assert_one_graph(p2p, ref, kw)


def _full_params(results):
    """The full model from the stages of DP replica 0 (a split head: the vocab parts in order)."""
    pieces = {}
    for r in results:
        if r["dp_idx"] != 0:
            continue
        for n, t in r["named"].items():
            pieces.setdefault(n, {})[r["head_part"][0] if n.startswith("lm_head") else 0] = t
    return {n: torch.cat([p[k] for k in sorted(p)], 0) for n, p in pieces.items()}


def test_global_clip_four_stages_matches_single_gpu(cuda):
    """S = 4, pp_clip: global: the norm is a four-term fp32 sum in rank order, gloo's is in another order, so the
    reference is the single-process run (loss rel / abs 2e-2, relative update error < 0.15)."""
    from distributed_training_compare_jax_amd.models.params import all_param_specs, init_full

    kw = {"pp_microbatches": 4, "pp_schedule": "1f1b", "pp_clip": "global", "pp_comm": "p2p"}
    res = _run("pp", 4, tuple(sorted(kw.items())))
    single = _run("dp", 1, ())
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=2e-2, abs=2e-2), (res[0]["losses"],
                                                                                         single[0]["losses"])
    for r in res:
        assert r["graphs"] == 1 and r["comms"] == 0, (r["pp_idx"], r["graphs"], r["comms"])
        assert r["losses"] == res[0]["losses"]
    p0 = {sp.name: init_full(sp, 0) for sp in all_param_specs(_model_cfg())}
    full, one = _full_params(res), _full_params(single)
    assert set(full) == set(one)
    for n in one:
        a, b, q = full[n], one[n], p0[n]
        if n.endswith("qkv.b"):  # key bias: analytically zero gradient, Adam normalises its noise
            a, b, q = (x.view(3, -1)[[0, 2]] for x in (a, b, q))
        err = (((a - q) - (b - q)).norm() / ((b - q).norm() + 1e-12)).item()
        assert err < 0.15, f"{n}: update differs from the single-GPU run by {err:.3f} (relative)"


def test_hybrid_dp2_pp2_matches_rccl_bitwise(cuda):
    """dp2 x pp2, 4 processes: the DP bucket collectives still cut the graph, the stage messages do not."""
    kw = {"dp": 2, "pp": 2, "pp_microbatches": 2, "pp_schedule": "1f1b"}
    p2p, ref = _pair(4, kw)
    _assert_bitwise(p2p, ref, kw)
    # what is left between the segments are the DP collectives and their waits, which the rccl run issues too, next
    # to its message exchanges (the segment count itself may go either way: empty segments are dropped)
    print(f"PP-P2P {kw}: p2p graphs/comms per rank {[(r['graphs'], r['comms']) for r in p2p]}, "
          f"rccl {[(r['graphs'], r['comms']) for r in ref]}")
    assert all(a["comms"] < b["comms"] for a, b in zip(p2p, ref)), \
        [(a["graphs"], a["comms"], b["graphs"], b["comms"]) for a, b in zip(p2p, ref)]
    for a, b in ((0, 1), (2, 3)):  # the two replicas of a stage stay bit-identical
        assert torch.equal(p2p[a]["params"], p2p[b]["params"])


def test_debug_build_runs_the_pipe_asserts_clean(cuda):
    """One pp2 case on the -DDTC_DEBUG library (every DTC_ASSERT of the message kernels live), selected with
    DTC_KERNEL_LIB in the spawned ranks as tests/test_debug_build_gpu.py does in its child processes."""
    dbg = os.path.join(PKG, "_dtc_kernels_debug.so")
    assert os.path.exists(dbg), "debug kernel library missing: __graft_entry__.build() builds it in-tree"
    kw = {"pp_microbatches": 2, "pp_schedule": "1f1b", "pp_comm": "p2p"}
    res = _run("pp", 2, tuple(sorted(dict(kw, kernel_lib=dbg).items())))
    rel = _run("pp", 2, tuple(sorted(kw.items())))
    assert all(r["lib"] == dbg for r in res) and all(r["lib"] != dbg for r in rel)
    assert all(r["graphs"] == 1 and r["comms"] == 0 for r in res)
    # -O1 kernels round like the release ones up to the GEMMs' accumulation order
    assert res[0]["losses"] == pytest.approx(rel[0]["losses"], rel=2e-2, abs=2e-2)
