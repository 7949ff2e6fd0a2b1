"""``Engine.evaluate`` on the HIP path, one process: the evaluation loss IS the training forward's loss on the same rows
(dropout 0) and the top-1 the arg-max of that forward's stored logits; interleaving evaluations leaves five training
steps bit for bit as they were; the evaluation program is one hipGraph; repeated evaluations agree; the peak memory
stays below a training step's and does not grow with the depth; ``main.py --eval_every`` writes ``eval.csv``.
(The multi-rank layouts: ``tests/test_eval_dist_gpu.py``.)"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset, replace
from distributed_training_compare_jax_amd.data import synthetic
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 8

# (TrainConfig fields, ModelConfig overrides): the MXFP8 GEMM's k-step wants d_model and d_ff multiples of 128
CASES = {
    "bf16": ({}, {}),
    "grad_accum2": (dict(grad_accum=2), {}),
    "mxfp8": (dict(fwd_gemm_dtype="mxfp8"), dict(d_model=128, d_ff=512, max_seq_len=128)),
    "fp32": (dict(dtype="fp32"), {}),
}


def _engine(dev, case, use_graph=True, layers=2, **kw):
    tkw, mkw = CASES[case]
    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=layers, **mkw)  # dropout 0.1
    tc = TrainConfig(seed=0, parallel="dp", batch=BATCH, steps=5, log_every=1, output_dir="/tmp/x", use_graph=use_graph,
                     **dict(tkw, **kw))
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


def _train(eng, mc, steps, eval_every=0, n_eval=2):
    it = synthetic.get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
    losses, evals = [], []
    for s in range(1, steps + 1):
        eng.set_batch(next(it))
        eng.run_step()
        losses.append(eng.loss_value())
        if eval_every and s % eval_every == 0:
            evals.append(eng.evaluate(n_eval))
    torch.cuda.synchronize()
    return losses, evals


def _heldout(mc, i):
    s = synthetic.SyntheticTokenStream(vocab=999, seed=0)
    rows = synthetic.heldout_rows(s, i, 0, BATCH, BATCH, mc.max_seq_len + 1)
    return (torch.from_numpy(rows[:, :-1]).contiguous().cuda(), torch.from_numpy(rows[:, 1:]).contiguous().cuda())


@pytest.mark.parametrize("case", ["bf16", "mxfp8", "fp32"])
def test_evaluate_is_the_training_forward(cuda, case):
    """One held-out batch: loss torch.equal to ``full_forward_loss`` on the same rows with dropout 0, top-1 the first
    arg-max over the valid columns of the logits that forward stored."""
    from distributed_training_compare_jax_amd.models.gpt import full_forward_loss
    from distributed_training_compare_jax_amd.ops import gemm as G
    from distributed_training_compare_jax_amd.ops import _native as N

    eng, mc = _engine(cuda, case, use_graph=False)
    _train(eng, mc, 1)
    out = eng.evaluate(1)
    if case != "fp32":  # the last bf16 GEMM of the evaluation is its head: the logits-free epilogue
        assert G.last_launch().epi == N.EPI_LMHEAD_EVAL
    ids, labels = _heldout(mc, 0)
    st = eng.stage
    cfg = st.cfg
    st.cfg = replace(cfg, dropout=0.0)
    try:
        loss, ctx = full_forward_loss(st, ids, labels, eng.opt.step_t)
    finally:
        st.cfg = cfg
    torch.cuda.synchronize()
    assert out["loss"] == float(loss.item()), (out["loss"], float(loss.item()))
    logits, lab = ctx["head"][4], ctx["head"][6]
    lg = logits[:, :mc.vocab_size].float()
    idx = torch.arange(lg.shape[1], device="cuda", dtype=torch.int32)
    first = torch.where(lg == lg.max(-1, keepdim=True).values, idx, torch.full_like(idx, 2**31 - 1)).min(-1).values
    tokens = BATCH * mc.max_seq_len
    assert out["tokens"] == tokens and round(out["top1"] * tokens) == int((first == lab).sum())
    assert out["ppl"] == pytest.approx(np.exp(out["loss"]), rel=1e-12)


@pytest.mark.parametrize("case", list(CASES))
def test_training_is_bit_identical_with_evaluation(cuda, case):
    """Five steps with an evaluation after steps 2 and 4 against five steps without: parameters, Adam moments, the
    compute-dtype mirror and the loss history are equal bit for bit, the training program has the same graphs, the
    evaluation program is ONE hipGraph with nothing eager in it, the step counter is where training left it."""
    off, mc = _engine(cuda, case)
    l0, _ = _train(off, mc, 5)
    on, _ = _engine(cuda, case)
    l1, evals = _train(on, mc, 5, eval_every=2)
    assert l1 == l0
    assert torch.equal(on.flat.params, off.flat.params)
    assert torch.equal(on.flat.exp_avg, off.flat.exp_avg) and torch.equal(on.flat.exp_avg_sq, off.flat.exp_avg_sq)
    assert case == "fp32" or torch.equal(on.flat.mirror, off.flat.mirror)  # (fp32 computes on the master copy)
    assert int(on.opt.step_t.item()) == int(off.opt.step_t.item()) == 5
    assert (on.program.n_graphs, on.program.n_comms) == (off.program.n_graphs, off.program.n_comms)
    assert off.eval_program is None and (on.eval_program.n_graphs, on.eval_program.n_comms) == (1, 0)
    assert len(evals) == 2 and all(np.isfinite(e["loss"]) and 0.0 <= e["top1"] <= 1.0 for e in evals)
    assert evals[0]["tokens"] == 2 * BATCH * mc.max_seq_len
    on.check_health()


def test_repeated_evaluations_agree(cuda):
    """With no training step between them: the first evaluation (its first batch eager, the second recorded and
    replayed) and the next two (replays only) return the same numbers, as does one over more batches for the shared
    prefix's worth of tokens."""
    eng, mc = _engine(cuda, "bf16")
    _train(eng, mc, 2)
    a, b, c = eng.evaluate(3), eng.evaluate(3), eng.evaluate(3)
    assert a == b == c
    one = [eng.evaluate(1) for _ in range(2)]
    assert one[0] == one[1] and one[0]["tokens"] * 3 == a["tokens"]


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_evaluation_peak_memory(cuda):
    """Eager, so that every tensor is a live allocation: the evaluation's peak above what was allocated on entry is
    below the training step's, and it does not grow with the depth (each layer's saved activations die as the layer
    returns: 6 layers peak within one residual-stream tensor of 2 layers; kept, they would add 4 layers' worth)."""
    peaks = {}
    for layers in (2, 6):
        eng, mc = _engine(cuda, "bf16", use_graph=False, layers=layers)
        it = synthetic.get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
        eng.set_batch(next(it))
        eng.run_step()
        eng.evaluate(1)  # (its buffers exist from here on)
        eng.set_batch(next(it))
        peaks[layers] = (_peak(eng.run_step), _peak(lambda: eng.evaluate(1)))
        del eng
    for layers, (train, ev) in peaks.items():
        assert 0 < ev < train, (layers, ev, train)
    resid = BATCH * 64 * 64 * 4  # rows x d_model fp32
    assert peaks[6][1] <= peaks[2][1] + resid, peaks


def test_main_writes_eval_csv(cuda, tmp_path):
    out = tmp_path / "dp"
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--train_config_path", "configs/train_config_dp.yaml",
           "--model_config_path", "configs/model_config_tiny.yaml", "--nproc", "1", "--steps", "5", "--warmup_steps", "1",
           "--log_every", "1", "--eval_every", "2", "--eval_batches", "2", "--output_dir", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("Eval: ")]
    assert len(lines) == 3 and lines[0].startswith("Eval: 1 | loss: ") and " | ppl: " in lines[0] \
        and " | top-1: " in lines[0] and " | time: " in lines[0], r.stdout
    ev = open(out / "eval.csv").read().strip().split("\n")
    assert ev[0] == "step,elapsed_time,eval_loss,eval_ppl,eval_top1,eval_time"
    assert [int(l.split(",")[0]) for l in ev[1:]] == [0, 2, 4]
    for l in ev[1:]:
        _, el, loss, ppl, top1, dt = (float(x) for x in l.split(","))
        assert ppl == pytest.approx(np.exp(loss), rel=1e-9) and 0.0 <= top1 <= 1.0 and dt > 0 and 3.0 < loss < 12.0
    log = open(out / "log.csv").read().strip().split("\n")  # the reference's format, untouched
    assert log[0] == "step,elapsed_time,loss" and len(log) == 6 and all(len(l.split(",")) == 3 for l in log)
    assert [l for l in r.stdout.split("\n") if l.startswith("Step: ")][0].startswith("Step: 1 | Avg loss: ")
    m = json.load(open(out / "metrics.json"))
    assert m["eval_last"]["step"] == 5 and m["eval_time_total_s"] > 0
