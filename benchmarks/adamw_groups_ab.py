"""A/B of ``FusedAdamW.step()`` with and without parameter groups on the real flat layouts.

    python benchmarks/adamw_groups_ab.py [--models gpt2-small,gpt-1.3b] [--rounds 7] [--reps 5] [--flat] [--out FILE]

Per model: the flat buffers of the whole model (no model is run: random parameters and gradients), the bf16 mirror and
the transposed mirror of fc1 / qkv / out_proj / lm_head as the engine keeps them, and two ``FusedAdamW`` over the SAME
buffers: one without groups (the ungrouped kernels) and one under the decay-mask rule ``["*.b", "*.g"] -> weight_decay
0`` (the grouped kernels, segments split at the run bounds).  A step is the global norm + the AdamW launches, timed
with device events.  The buffers are 2.6 GB (GPT-2 small) and 21 GB (1.3B) per pass, far beyond the caches, so every
step is HBM-cold by size.  The two variants alternate inside each round; a round's figure is the mean of ``--reps``
steps; the table gives min / median / max over the rounds, so the spread is this measurement's own.  ``--flat``
keeps no transposed mirror, so the step takes ``adamw_kernel`` over the whole buffer (the kernel the ZeRO-1 slices and
the deferred optimizer use) instead of the segmented + tiled pair.

Prints one JSON line per (model, variant) (and appends them to ``--out``)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_training_compare_jax_amd.config.schema import OptimConfig, model_config_from_preset  # noqa: E402
from distributed_training_compare_jax_amd.models.params import all_param_specs  # noqa: E402
from distributed_training_compare_jax_amd.ops import optim as O  # noqa: E402
from distributed_training_compare_jax_amd.parallel.buffers import FlatParams  # noqa: E402
from distributed_training_compare_jax_amd.train.optimizer import FusedAdamW  # noqa: E402

MASK = [dict(match=["*.b", "*.g"], weight_decay=0.0)]


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def time_steps(opt, reps):
    """Mean ms of ``reps`` consecutive steps (device events around the lot)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        opt.step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def model(name, rounds, reps, out, flat_only=False):
    dev = torch.device("cuda")
    mc = model_config_from_preset(name)
    flat = FlatParams(all_param_specs(mc), 0, 1, dev, compute_dtype=torch.bfloat16)
    if not flat_only:
        flat.enable_transposed([f"h.{l}.{n}.w" for l in range(mc.n_layers) for n in ("fc1", "qkv", "out")]
                               + ["lm_head.w"])
    g = torch.Generator(device=dev).manual_seed(0)
    for buf, scale in ((flat.params, 0.02), (flat.grads, 1e-3)):
        for lo in range(0, flat.numel, 1 << 28):  # in pieces: no second buffer-sized temporary
            hi = min(lo + (1 << 28), flat.numel)
            buf[lo:hi].normal_(0.0, scale, generator=g)
    flat.refresh_mirror()
    opts = {"ungrouped": FusedAdamW(flat, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), None),
            "decay_mask": FusedAdamW(flat, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0, param_groups=MASK),
                                     None)}
    info = {}
    for k, opt in opts.items():  # warmup: builds the launch plans; the record says which kernels a step takes
        time_steps(opt, 2)
        rec = O.last_adamw()
        assert rec["groups"] == (k == "decay_mask"), rec
        info[k] = rec
    t = {k: [] for k in opts}
    for _ in range(rounds):
        for k, opt in opts.items():
            t[k].append(time_steps(opt, reps))
    n_t = sum(sl.numel for sl, _ in flat.mirror_t.values())
    # per step: the norm reads g; the update reads p, g, m, v and writes p, m, v, the bf16 mirror and W^T
    nbytes = 4 * flat.numel + 28 * flat.numel + 2 * flat.n_mirror + 2 * n_t
    for k in opts:
        lo, med, hi = min(t[k]), statistics.median(t[k]), max(t[k])
        plan = opts[k]._aw_plans.get((0, flat.numel)) or []
        emit(dict(bench="adamw_groups_ab", model=name, variant=k, path="flat" if flat_only else "tiled",
                  numel=flat.numel, bytes_per_step=nbytes,
                  runs=info[k]["runs"], entry=info[k]["entry"], adamw_launches=info[k]["launches"],
                  norm_launches=2, segments=sum(sb.nseg for sb, _ in plan), tiles=sum(tb.ntasks for _, tb in plan),
                  rounds=rounds, reps=reps, ms_min=round(lo, 4), ms_median=round(med, 4), ms_max=round(hi, 4),
                  gbytes_per_s_median=round(nbytes / med / 1e6, 1)), out)
    a, b = statistics.median(t["ungrouped"]), statistics.median(t["decay_mask"])
    emit(dict(bench="adamw_groups_ab", model=name, variant="delta", ms=round(b - a, 4),
              percent=round(100 * (b - a) / a, 3),
              spread_ungrouped_ms=round(max(t["ungrouped"]) - min(t["ungrouped"]), 4),
              spread_decay_mask_ms=round(max(t["decay_mask"]) - min(t["decay_mask"]), 4)), out)
    del opts, flat
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gpt2-small,gpt-1.3b")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flat", action="store_true", help="no transposed mirror: adamw_kernel over the whole buffer")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5, "at least 5 rounds after the warmup"
    for name in a.models.split(","):
        model(name, a.rounds, a.reps, a.out, a.flat)


if __name__ == "__main__":
    main()
