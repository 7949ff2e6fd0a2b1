"""A/B of the evaluation head against the training head, and of an evaluation batch against the training forward.

    python benchmarks/eval_head_ab.py [--models gpt2-small,ref] [--rounds 7] [--reps 10] [--out FILE]

Part 1, per model: the lm_head GEMM at the model's training shape (8 sequences: 8192 x 50304 x 768 for GPT-2 small,
4096 x 50304 x 512 for the reference model) with the storing epilogue (``EPI_LMHEAD``: bf16 logits + row statistics)
and with the evaluation epilogue (``EPI_LMHEAD_EVAL``: the statistics + the row arg-max, no logits), each followed by
what finishes it (``ce_finalize``; for the evaluation also ``ce_eval_finish``), and the GEMM launches alone.  HBM-cold:
every call follows a 512 MB buffer write whose own time is subtracted (the method of ``benchmarks/gemm_layer_ab.py
--cold``); rounds alternate the two, the table gives min / median / max over the rounds, so the spread is the
run-to-run spread of this very measurement.

Part 2, per model: one evaluation batch (``Engine._eval_fn`` captured as its hipGraph) against the training forward
alone (embedding with dropout, blocks, storing head; captured the same way) on the same engine, alternating.

Prints one JSON line per row (and appends them to ``--out``)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_layer_ab import graph_time  # noqa: E402

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset  # noqa: E402
from distributed_training_compare_jax_amd.ops import _native as N  # noqa: E402
from distributed_training_compare_jax_amd.ops import gemm as G  # noqa: E402
from distributed_training_compare_jax_amd.ops import xent as X  # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def ab(variants, rounds, reps, pre):
    """variants: name -> fn.  Interleaved rounds; us per call, (min, median, max) per variant."""
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(graph_time(fn, reps, pre))
    return {k: (min(v), statistics.median(v), max(v)) for k, v in t.items()}


def head(model, rounds, reps, out):
    mc = model_config_from_preset(model)
    dev = torch.device("cuda")
    M, D, V, Vp = 8 * mc.max_seq_len, mc.d_model, mc.vocab_size, mc.padded_vocab
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(M, D, device=dev, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(Vp, D, device=dev, generator=g)).to(torch.bfloat16)
    b = 0.1 * torch.randn(Vp, device=dev, generator=g)
    labels = torch.randint(0, V, (M,), device=dev, dtype=torch.int32, generator=g)
    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    pre = lambda: flush.fill_(1.0)  # noqa: E731
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def store():
        return X.lmhead_logits_partials(h, w, b, labels, 0, V, combine=False)

    def store_fin():
        _, part, lab = store()
        return X.ce_finalize(part, lab, 1.0 / M)

    def ev():
        return X.lmhead_eval_partials(h, w, b, labels, 0, V)

    def ev_fin():
        part, lab, cv, cc = ev()
        X.ce_eval_finish(cv, cc, 0, labels, count)
        return X.ce_finalize(part, lab, 1.0 / M)

    store()
    fam_s = G.last_launch()
    ev()
    fam_e = G.last_launch()
    assert fam_s.family == fam_e.family and fam_s.epi == N.EPI_LMHEAD and fam_e.epi == N.EPI_LMHEAD_EVAL
    res = ab({"store": store, "eval": ev, "store+finalize": store_fin, "eval+finish+finalize": ev_fin}, rounds, reps, pre)
    for k, (lo, med, hi) in res.items():
        emit(dict(part="head", model=model, shape=[M, Vp, D], family=fam_s.family, variant=k, us_min=round(lo, 1),
                  us_median=round(med, 1), us_max=round(hi, 1), logits_mb=round(M * Vp * 2 / 1e6, 1)), out)


def batch(model, rounds, reps, out):
    from distributed_training_compare_jax_amd.data import synthetic
    from distributed_training_compare_jax_amd.models.gpt import full_forward_loss
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine

    dev = torch.device("cuda", 0)
    mc = model_config_from_preset(model)
    tc = TrainConfig(seed=0, parallel="dp", batch=8, steps=1, log_every=1, output_dir="/tmp/x", use_graph=False)
    eng = Engine(mc, tc, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl"))
    eng.set_batch(next(synthetic.get_batch_iterator(8, mc.max_seq_len + 1)))
    eng.run_step()
    eng.loss_value()
    eng.evaluate(1)  # (its static inputs hold held-out batch 0 from here on)
    st = eng.stage

    def fwd_train():
        loss, ctx = full_forward_loss(st, eng.ids, eng.labels, eng.opt.step_t)
        return loss

    res = ab({"training forward": fwd_train, "evaluation batch": eng._eval_fn}, rounds, max(1, reps // 3), None)
    for k, (lo, med, hi) in res.items():
        emit(dict(part="batch", model=model, rows=8 * mc.max_seq_len, variant=k, us_min=round(lo, 1),
                  us_median=round(med, 1), us_max=round(hi, 1)), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gpt2-small,ref")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="head,batch")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_head_ab.py measures on the GPU: no device found")
    for m in a.models.split(","):
        if "head" in a.parts:
            head(m, a.rounds, a.reps, a.out)
        if "batch" in a.parts:
            batch(m, a.rounds, a.reps, a.out)


if __name__ == "__main__":
    main()
