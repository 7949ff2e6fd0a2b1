"""``Engine.evaluate`` under the multi-rank layouts, on the rig of tests/test_dist_gpu.py (2 processes share cuda:0 over
gloo; the peer-to-peer transports run for real over IPC mappings): five training steps with an evaluation after steps
2 and 4 are bit for bit the five steps without one -- parameters, Adam moments, the bf16 mirror, the loss history, the
training program's graphs -- and every transport's ``check()`` passes after the interleaving (the evaluation program
pads its own P2P calls to an even count); under ``tp_comm: p2p`` the evaluation program is one hipGraph with nothing
eager in it; the DP sum of an evaluation is the one eager collective; dp 2 and dp 1 evaluate identical parameters to
the same count and, within the fp32 sum's bound, the same loss."""

import functools
import os
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
STEPS, BATCH, N_EVAL = 5, 4, 2
U24 = 2.0 ** -24


def _worker(parallel, kw, eval_every, lr, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.engine import Engine

    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=2)
    tc = TrainConfig(seed=0, parallel=parallel, batch=BATCH, steps=STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cuda", warmup_steps=0, **kw)
    d = init_distributed("cuda")
    eng = Engine(mc, tc, OptimConfig(lr=lr, weight_decay=0.1, grad_clip=1.0), d)
    it = get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999, row0=eng.feed_row0, nrows=eng.feed_rows)
    calls = []
    real = dist.all_reduce

    def counting(t, *a, **k):  # eager process-group all-reduces issued while an evaluation runs
        calls.append((tuple(t.shape), str(t.dtype)))
        return real(t, *a, **k)

    losses, evals, eager = [], [], []
    for s in range(1, STEPS + 1):
        eng.set_batch(next(it))
        eng.run_step()
        losses.append(eng.loss_value())
        if eval_every and s % eval_every == 0:
            calls.clear()
            dist.all_reduce = counting
            try:
                evals.append(eng.evaluate(N_EVAL))
            finally:
                dist.all_reduce = real
            eager.append(list(calls))
    torch.cuda.synchronize()
    eng.check_health()  # every transport's check(): barrier words and the P2P buffer-half invariant
    ep = eng.eval_program
    torch.save({"losses": losses, "evals": evals, "eager": eager, "graphs": eng.program.n_graphs,
                "comms": eng.program.n_comms, "eval_graphs": None if ep is None else (ep.n_graphs, ep.n_comms),
                "params": eng.flat.params.cpu(), "m": eng.flat.exp_avg.cpu(), "v": eng.flat.exp_avg_sq.cpu(),
                "mirror": eng.flat.mirror.cpu(), "step": int(eng.opt.step_t.item()), "sp": eng.stage.sp,
                "p2p": [n for n, _ in eng._live_transports()]},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


@functools.lru_cache(maxsize=None)
def _run(parallel, world, kw_items, eval_every, lr=3e-3):
    with tempfile.TemporaryDirectory() as td:
        if world == 1:
            for k in ("WORLD_SIZE", "RANK"):
                os.environ.pop(k, None)
            _worker(parallel, dict(kw_items), eval_every, lr, td)
        else:
            spawn(_worker, world, args=(parallel, dict(kw_items), eval_every, lr, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(world)]


LAYOUTS = {
    "tp2_p2p": ("tp", dict(tp_comm="p2p", tp_sequence_parallel=False), "p2p"),
    "tp2_p2p_sp": ("tp", dict(tp_comm="p2p", tp_sequence_parallel=True), "p2p"),
    "dp2_p2p": ("dp", dict(dp_comm="p2p"), "dp_p2p"),
    "dp2_zero_p2p": ("dp", dict(zero_stage=1, zero_comm="p2p"), "dp_p2p"),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_training_is_bit_identical_with_evaluation(cuda, layout):
    parallel, kw, transport = LAYOUTS[layout]
    key = tuple(sorted(kw.items()))
    off, on = _run(parallel, 2, key, 0), _run(parallel, 2, key, 2)
    for a, b in zip(off, on):
        assert transport in b["p2p"] and b["sp"] == bool(kw.get("tp_sequence_parallel", False))
        assert a["losses"] == b["losses"], (a["losses"], b["losses"])
        for k in ("params", "m", "v", "mirror"):
            assert torch.equal(a[k], b[k]), (layout, k, int((a[k] != b[k]).sum()))
        assert a["step"] == b["step"] == STEPS
        assert (a["graphs"], a["comms"]) == (b["graphs"], b["comms"])
        assert a["eval_graphs"] is None and len(b["evals"]) == 2
    assert on[0]["evals"] == on[1]["evals"]  # every rank returns the same numbers
    for r in on:
        if parallel == "tp":  # in-graph TP collectives: ONE hipGraph, nothing eager, not even a DP sum
            assert r["eval_graphs"] == (1, 0) and r["eager"] == [[], []], (r["eval_graphs"], r["eager"])
        else:  # the float64 DP sum is the only eager collective, once per evaluation
            assert r["eval_graphs"] == (1, 0) and r["eager"] == [[((3,), "torch.float64")]] * 2, r["eager"]


def test_dp2_evaluates_what_dp1_evaluates(cuda):
    """Identical parameters (lr = 0: the canonical init, after the training steps the evaluation waits for): the same
    held-out rows as one replica of 4 rows per batch or two of 2.

    The correct count is an integer sum over the same rows: equal.  The loss differs only in how each batch's fp32
    sum of the per-row (lse - label logit) is taken (``ce_loss_reduce``: M rows over 1024 threads x 8 accumulators, a
    chain of ceil(M / 8192) additions per accumulator, 3 to fold the 8, 6 wave shuffles, 16 serial adds over the waves,
    then one multiply by the scale; each term carries the subtraction's own rounding): every term is >= 0, so each
    sum is within gamma_d = d u / (1 - d u), d = ceil(M / 8192) + 3 + 6 + 16 + 2, u = 2^-24, of the exact sum of its
    rows (derived as tests/test_zero_p2p_gpu.py ``sumsq_bound`` does for its partials); what follows -- the float64
    sums over batches and ranks -- is exact to 2^-53.  Both layouts are within gamma_d of the same exact mean."""
    one = _run("dp", 1, (), 2, 0.0)[0]
    two = _run("dp", 2, (), 2, 0.0)
    assert two[0]["evals"] == two[1]["evals"]
    M = BATCH * 64  # the larger per-rank row count (dp 1)
    d = (-(-M // 8192) + 3 + 6 + 16 + 2) * U24
    gamma = d / (1 - d)
    for a, b in zip(one["evals"], two[0]["evals"]):
        assert a["tokens"] == b["tokens"] == N_EVAL * BATCH * 64
        assert round(a["top1"] * a["tokens"]) == round(b["top1"] * b["tokens"])
        err = abs(a["loss"] - b["loss"])
        print(f"EVAL dp1 {a['loss']!r} dp2 {b['loss']!r} err {err:.3e} bound {2 * gamma * a['loss']:.3e}")
        assert err <= 2 * gamma * a["loss"]
    assert one["evals"][0] == one["evals"][1]  # lr 0: the same model at both evaluations
