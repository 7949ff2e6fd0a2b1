"""Held-out evaluation without a GPU: the config fields and their refusals, the held-out rows, the CPU engine's
``evaluate()`` against the autograd oracle, that evaluating leaves the training run bit for bit untouched (one process,
and gloo ranks at dp 2 and tp 2), and the arg-max semantics the GPU epilogue is held to."""

import math
import os
import tempfile

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data import synthetic
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn

STEPS = 5


def _cfgs(parallel="dp", eval_every=0, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel=parallel, batch=4, steps=STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cpu", warmup_steps=0, eval_every=eval_every, eval_batches=2, **kw)
    oc = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0)
    return mc, tc, oc


def _tc(**kw):
    return TrainConfig(seed=0, parallel="dp", batch=4, steps=10, log_every=1, output_dir="/tmp/unused", **kw)


# ------------------------------------------------------------------------------------------ schema
def test_schema_defaults_and_yaml(tmp_path):
    from distributed_training_compare_jax_amd.config.schema import build_configs

    tc = _tc()
    assert tc.eval_every == 0 and tc.eval_batches == 8
    y = tmp_path / "t.yaml"
    y.write_text(open("configs/train_config_dp.yaml").read() + "\neval_every: 50\neval_batches: 3\n")
    tc, _, _ = build_configs(str(y))
    assert (tc.eval_every, tc.eval_batches) == (50, 3)


@pytest.mark.parametrize("kw,word", [
    (dict(eval_every=-1), "eval_every"),
    (dict(eval_batches=-2), "eval_batches"),
    (dict(eval_every=True), "eval_every"),
    (dict(eval_every=2, eval_batches=0), "eval_batches"),
    (dict(eval_every=2, defer_optimizer=True), "defer_optimizer"),
    (dict(eval_every=2, pp=2), "pipeline"),
    (dict(eval_every=2, data="fineweb"), "synthetic"),
])
def test_schema_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        _tc(**kw)
    # the same fields with evaluation off are none of its business
    off = {k: v for k, v in kw.items() if not k.startswith("eval_")}
    if off:
        _tc(**off)


def test_engine_refuses_pipelines_and_reachable_positions():
    from distributed_training_compare_jax_amd.train.engine import Engine

    mc, tc, oc = _cfgs("pp", eval_every=2)
    dinfo = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")
    Engine(mc, tc, oc, dinfo)  # parallel: pp on one rank is pp = 1
    eng = Engine(*_cfgs("dp"), dinfo)
    with pytest.raises(RuntimeError, match="first training step"):
        eng.evaluate(1)
    # steps x batch x seq_len reaching the held-out base: refused before anything is built
    steps = synthetic.EVAL_POS_BASE // (4 * (mc.max_seq_len + 1)) + 1
    tc_far = TrainConfig(seed=0, parallel="dp", batch=4, steps=steps, log_every=1, output_dir="/tmp/unused", device="cpu",
                         warmup_steps=0, eval_every=100)
    with pytest.raises(ValueError, match="held-out"):
        Engine(mc, tc_far, oc, dinfo)
    synthetic.check_heldout_disjoint(steps - 1, 4, mc.max_seq_len + 1)
    with pytest.raises(ValueError, match="held-out"):
        synthetic.check_heldout_disjoint(steps, 4, mc.max_seq_len + 1)


# ------------------------------------------------------------------------------------------ held-out rows
def test_heldout_rows_fixed_layout_invariant_and_disjoint():
    B, L = 8, 65
    s = synthetic.SyntheticTokenStream(vocab=999, seed=3)
    full = [synthetic.heldout_rows(s, i, 0, B, B, L) for i in range(3)]
    again = [synthetic.heldout_rows(synthetic.SyntheticTokenStream(vocab=999, seed=3), i, 0, B, B, L) for i in range(3)]
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    assert not np.array_equal(full[0], full[1])
    for i in range(3):  # the dp2 row slices concatenate to dp1's; any rank generates only its rows
        halves = [synthetic.heldout_rows(s, i, r0, B // 2, B, L) for r0 in (0, B // 2)]
        assert np.array_equal(np.concatenate(halves), full[i])
    # the native sampler and the numpy path agree out there too
    assert np.array_equal(s.tokens_numpy(synthetic.EVAL_POS_BASE, 300), s.tokens(synthetic.EVAL_POS_BASE, 300))
    # positions: evaluation rows start at the base; a configured run's training rows end below it
    steps = 1000
    last_train_pos = (steps * B) * L - 1
    assert last_train_pos < synthetic.EVAL_POS_BASE
    synthetic.check_heldout_disjoint(steps, B, L)
    # and the tokens differ from the training batches' (same stream, other positions)
    assert not any(np.array_equal(full[0], s.rows(t, 0, B, B, L)) for t in range(4))


# ------------------------------------------------------------------------------------------ engine vs oracle
def _trained_engine(**kw):
    from distributed_training_compare_jax_amd.train.loop import train

    mc, tc, oc = _cfgs(**kw)
    r = train(tc, mc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"), quiet=True, write_csv=False)
    return mc, r


def test_cpu_engine_evaluate_matches_the_oracle():
    """loss: |engine - oracle| < 1e-5, the bound of tests/test_model_cpu.py::test_explicit_backward_matches_autograd
    (the CPU engine against the same oracle); top-1: the oracle's arg-max, on every row whose top two oracle logits
    are further apart than that bound (closer ones may legitimately order either way in fp32)."""
    from distributed_training_compare_jax_amd.models.reference import oracle_logits

    mc, r = _trained_engine()
    eng = r["engine"]
    n = 2
    out = eng.evaluate(n)
    T = mc.max_seq_len
    stream = synthetic.SyntheticTokenStream(vocab=min(synthetic.BPE_VOCAB, mc.vocab_size - 1), seed=0)
    params = {k: eng.flat.p(k).clone() for k in eng.flat.slots}
    mc0 = model_config_from_preset("tiny", vocab_size=1000, dropout=0.0)
    loss_sum, hits, unsure = 0.0, 0, 0
    for i in range(n):
        rows = synthetic.heldout_rows(stream, i, 0, 4, 4, T + 1)
        ids, lab = torch.from_numpy(rows[:, :-1]).contiguous(), torch.from_numpy(rows[:, 1:]).contiguous()
        logits = oracle_logits(mc0, params, ids, 0, 0).reshape(-1, mc.vocab_size)
        loss_sum += float(torch.nn.functional.cross_entropy(logits, lab.reshape(-1).long(), reduction="sum"))
        top2 = logits.topk(2, -1).values
        unsure += int(((top2[:, 0] - top2[:, 1]) < 1e-5).sum())
        hits += int((logits.argmax(-1) == lab.reshape(-1)).sum())
    tokens = n * 4 * T
    assert out["tokens"] == tokens
    assert abs(out["loss"] - loss_sum / tokens) < 1e-5
    assert out["ppl"] == pytest.approx(math.exp(out["loss"]), rel=1e-12)
    assert abs(out["top1"] * tokens - hits) <= unsure
    assert eng.evaluate(n) == out  # nothing between them: identical


# ------------------------------------------------------------------------------------------ training untouched
def test_training_is_bit_identical_with_evaluation_cpu(tmp_path):
    _, a = _trained_engine(eval_every=0)
    _, b = _trained_engine(eval_every=2)
    assert a["history"] == b["history"]
    ea, eb = a["engine"], b["engine"]
    assert torch.equal(ea.flat.params, eb.flat.params)
    assert torch.equal(ea.flat.exp_avg, eb.flat.exp_avg) and torch.equal(ea.flat.exp_avg_sq, eb.flat.exp_avg_sq)
    assert [s for s, _ in b["evals"]] == [2, 4, 5] and a["evals"] == []
    assert "eval_last" not in a and b["eval_last"]["step"] == 5 and b["eval_time_total_s"] > 0
    losses = [r["loss"] for _, r in b["evals"]]
    assert losses[-1] < losses[0]  # the held-out loss falls with training (same stream structure)


def test_loop_writes_eval_csv_and_keeps_log_csv(tmp_path):
    from distributed_training_compare_jax_amd.train.loop import train

    mc, tc, oc = _cfgs(eval_every=2)
    from dataclasses import replace

    tc = replace(tc, output_dir=str(tmp_path), log_every=1)
    train(tc, mc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"), quiet=True)
    ev = open(tmp_path / "eval.csv").read().strip().split("\n")
    assert ev[0] == "step,elapsed_time,eval_loss,eval_ppl,eval_top1,eval_time"
    assert [int(l.split(",")[0]) for l in ev[1:]] == [1, 3, 4]  # the log.csv rows the evaluations follow
    log = open(tmp_path / "log.csv").read().strip().split("\n")
    assert log[0] == "step,elapsed_time,loss" and len(log) == 1 + STEPS
    el = [float(l.split(",")[1]) for l in log[1:]]
    assert all(b > a for a, b in zip(el, el[1:]))
    import json

    m = json.load(open(tmp_path / "metrics.json"))
    assert m["eval_last"]["step"] == 5 and set(m["eval_last"]) == {"step", "loss", "ppl", "top1", "tokens"}
    # with evaluation off: no eval.csv, no new metrics keys
    tc0 = replace(tc, eval_every=0, output_dir=str(tmp_path / "off"))
    train(tc0, mc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"), quiet=True)
    assert not os.path.exists(tmp_path / "off" / "eval.csv")
    m0 = json.load(open(tmp_path / "off" / "metrics.json"))
    assert set(m) - set(m0) == {"eval_last", "eval_time_total_s"}


def _worker(parallel, eval_every, kw, out_dir):
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    torch.set_num_threads(1)
    mc, tc, oc = _cfgs(parallel, eval_every=eval_every, **kw)
    d = init_distributed("cpu")
    r = train(tc, mc, oc, d, quiet=True, write_csv=False)
    eng = r["engine"]
    torch.save({"losses": r["history"], "params": eng.flat.params.clone(), "m": eng.flat.exp_avg.clone(),
                "v": eng.flat.exp_avg_sq.clone(), "evals": r["evals"]}, os.path.join(out_dir, f"rank{d.rank}.pt"))
    destroy()


def _spawned(parallel, eval_every, **kw):
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, 2, args=(parallel, eval_every, kw, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(2)]


@pytest.mark.slow
@pytest.mark.parametrize("parallel,kw", [("dp", {}), ("tp", {"tp_sequence_parallel": False}),
                                         ("tp", {"tp_sequence_parallel": True})],
                         ids=["dp2", "tp2", "tp2_sp"])
def test_training_is_bit_identical_with_evaluation_gloo(parallel, kw):
    off, on = _spawned(parallel, 0, **kw), _spawned(parallel, 2, **kw)
    for a, b in zip(off, on):
        assert a["losses"] == b["losses"]
        for k in ("params", "m", "v"):
            assert torch.equal(a[k], b[k]), k
    assert on[0]["evals"] == on[1]["evals"] and len(on[0]["evals"]) == 3  # every rank holds the same numbers
    # and they are the single-process evaluation of the same model, up to the layouts' fp32 summation order (the
    # bound tests/test_parallel_cpu.py::test_layout_matches_single_process puts on the losses of the same layouts)
    _, single = _trained_engine(eval_every=2)
    for (s1, r1), (s2, r2) in zip(single["evals"], on[0]["evals"]):
        assert s1 == s2 and r1["tokens"] == r2["tokens"]
        assert r2["loss"] == pytest.approx(r1["loss"], rel=1e-4, abs=1e-4)


# ------------------------------------------------------------------------------------------ arg-max semantics
def _emul(logits, labels, vocab_start, n_valid):
    """The CPU branch on given logits: h = I, w = logitsᵀ."""
    from distributed_training_compare_jax_amd.ops import xent as X

    M, Vl = logits.shape
    return X.lmhead_eval_partials(torch.eye(M), logits.t().contiguous(), torch.zeros(Vl), labels, vocab_start, n_valid)


def test_argmax_emulation_self_checks():
    from distributed_training_compare_jax_amd.ops import xent as X

    lg = torch.tensor([[1.0, 5.0, 5.0, 2.0, 9.0, 9.0],     # tie 1-2 among the valid; the pads are larger
                       [7.0, 7.0, 7.0, 7.0, 0.0, 0.0],     # all tied: the lowest
                       [0.0, 1.0, 2.0, 3.0, 3.0, 3.0]])    # valid max at 3, ties with pads
    labels = torch.tensor([1, 0, 4], dtype=torch.int32)
    part, lab, cval, ccol = _emul(lg, labels, 0, 4)
    assert ccol.tolist() == [[1, 0, 3]] and cval.tolist() == [[5.0, 7.0, 3.0]]
    assert torch.equal(part[0, :, 0], cval[0])  # the part maximum is the value at the arg-max
    count = torch.tensor([10], dtype=torch.int32)
    am, val, ok = X.ce_eval_finish(cval, ccol, 0, labels, count)
    assert am.tolist() == [1, 0, 3] and ok.tolist() == [1, 1, 0] and int(count) == 12
    # a shard with no valid column: no candidate, and it never wins the finish
    p0, l0, v0, c0 = _emul(lg, labels, 100, 0)
    assert c0.tolist() == [[-1, -1, -1]] and bool((v0 == float("-inf")).all())
    # two shards [0, 3) and [3, 6) with 4 valid columns in all: row 2's maximum lies in the second, row 0 ties inside
    # the first; equal values across shards go to the lower global column
    lg2 = lg.clone()
    lg2[1] = torch.tensor([7.0, 1.0, 1.0, 7.0, 0.0, 0.0])
    shards = [_emul(lg2[:, :3].contiguous(), labels, 0, 3), _emul(lg2[:, 3:].contiguous(), labels, 3, 1)]
    mine = [X.ce_eval_finish(s[2], s[3], off)[0] for s, off in zip(shards, (0, 3))]
    assert [m.tolist() for m in mine] == [[1, 0, 2], [3, 3, 3]]
    g = torch.stack([torch.cat([X.combine_partials(s[0]), m.float()[:, None]], 1) for s, m in zip(shards, mine)])
    count = torch.zeros(1, dtype=torch.int32)
    am, _, ok = X.ce_eval_finish(g[:, :, 0], g[:, :, 2], 0, labels, count)
    assert am.tolist() == [1, 0, 3] and int(count) == 2
    # rounding to the activation dtype happens before max / arg-max: two logits that differ only below bf16 tie
    a = torch.tensor([[1.0, 1.0 + 2.0 ** -10]])
    assert _emul(a.to(torch.bfloat16).float(), torch.tensor([0], dtype=torch.int32), 0, 2)[3].tolist() == [[0]]
    assert _emul(a, torch.tensor([0], dtype=torch.int32), 0, 2)[3].tolist() == [[1]]
