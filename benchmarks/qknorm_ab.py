"""The fused QK-norm + RoPE kernels (csrc/qknorm.hip) next to the RoPE kernel alone (csrc/rope.hip, the pass they
replace) on the same tensor, HBM-cold, and a training step with ``qk_norm: rmsnorm`` against ``none``.

    python benchmarks/qknorm_ab.py [--rounds 7] [--reps 16]      # kernels: forward and backward at two shapes
    python benchmarks/qknorm_ab.py --step [--model gpt2-small] [--steps 60] [--warmup 10] [--rounds 3]

Kernel mode, as benchmarks/rope_ab.py: gpt2-small (8192 tokens, H 12, hd 64) and gpt-1.3b-gqa (8 x 2048 tokens, H 16,
Hkv 4, hd 128), bf16; ``reps`` copies of every operand (more than 600 MB of activations, past the 256 MB last-level
cache) are visited in turn inside one captured graph, so every call reads from HBM; the time is the replay's device-
event time over ``reps``.  The fused kernels alternate with ``rope_`` (forward / inverse) in the same process.
Reported: the median time, bytes/s against each kernel's minimal traffic (n = rows * (H + Hkv) * hd * sizeof(T), r =
rows * (H + Hkv) * 4: rope 2 n; fused forward 3 n + r -- read n, write y and the raw copy; fused backward 3 n + r --
read dy, the raw copy and rstd, write dx), the share of the 8 TB/s HBM peak and the time over rope's.  The backward
figure includes its ordered slab reduction (a second, tiny launch).

Step mode: the engine loop of ``bench.py`` (8 sequences, one GPU, hipGraph) on ``--model`` (a preset name, or
``1p3b``: configs/model_config_gpt_1p3b_gqa_rope_rms_swiglu.yaml at batch 4) with ``pos_emb: rope`` and ``qk_norm`` none /
rmsnorm alternating; prints each run's ms/step, the spread and the difference per step.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_training_compare_jax_amd.ops import _native as NV  # noqa: E402
from distributed_training_compare_jax_amd.ops.qknorm import qknorm_rope_bwd_, qknorm_rope_fwd_  # noqa: E402
from distributed_training_compare_jax_amd.ops.rope import rope_, rope_table  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
SHAPES = {"gpt2-small": (8, 1024, 12, 12, 64), "gpt-1.3b-gqa": (8, 2048, 16, 4, 128)}  # B, T, H, Hkv, hd


def graph_time(fns):
    """us per call of the captured sequence ``fns`` (one replay warm, one timed)."""
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for f in fns:
            f()
    gr.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    gr.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / len(fns) * 1e3


def kernel_mode(a):
    dev = torch.device("cuda")
    for name, (B, T, H, Hkv, hd) in SHAPES.items():
        ld, nrot = (H + 2 * Hkv) * hd, H + Hkv
        reps = max(a.reps, -(-600 * 2 ** 20 // (B * T * ld * 2)))
        xs = [torch.randn(B, T, ld, device=dev).to(torch.bfloat16) for _ in range(reps)]
        tab = rope_table(T, hd, 10000.0, dev)
        gq, gk = torch.rand(hd, device=dev) + 0.5, torch.rand(hd, device=dev) + 0.5
        dgq, dgk = torch.zeros(hd, device=dev), torch.zeros(hd, device=dev)
        # saved tensors of the backward: one set per activation, written once (outside the timed graphs)
        saved = [qknorm_rope_fwd_(x.clone(), tab, gq, gk, H, Hkv, 1e-6)[1:] for x in xs]
        raws = [torch.empty_like(s[0]) for s in saved]
        rstds = [torch.empty_like(s[1]) for s in saved]

        def fwd(x, raw, rstd):  # the op's launch into preallocated outputs (no allocation inside the graph)
            NV.check(NV.lib().dtc_qknorm_fwd(x.data_ptr(), tab.data_ptr(), gq.data_ptr(), gk.data_ptr(), raw.data_ptr(),
                                             rstd.data_ptr(), B, T, H, Hkv, hd, T, 1e-6, 0, NV.stream_ptr(dev)),
                     "dtc_qknorm_fwd")

        runs = {"rope fwd": [lambda x=x: rope_(x, tab, H, Hkv) for x in xs],
                "rope inv": [lambda x=x: rope_(x, tab, H, Hkv, inverse=True) for x in xs],
                "qkn fwd": [lambda x=x, r=r, s=s: fwd(x, r, s) for x, r, s in zip(xs, raws, rstds)],
                "qkn bwd": [lambda x=x, s=s: qknorm_rope_bwd_(x, tab, s[0], s[1], gq, gk, H, Hkv, dgq, dgk)
                            for x, s in zip(xs, saved)]}
        for f in runs.values():
            f[0]()
        torch.cuda.synchronize()
        res = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, f in runs.items():
                res[k].append(graph_time(f))
        n, r = B * T * nrot * hd * 2, B * T * nrot * 4
        traffic = {"rope fwd": 2 * n, "rope inv": 2 * n, "qkn fwd": 3 * n + r, "qkn bwd": 3 * n + r}
        med = {k: statistics.median(v) for k, v in res.items()}
        for k, v in res.items():
            bw = traffic[k] / (med[k] * 1e-6)
            base = med["rope fwd" if k.endswith("fwd") else "rope inv"]
            print(f"{name:13s} {k:8s} {med[k]:7.1f} us (min {min(v):.1f} max {max(v):.1f}, {reps} tensors, {a.rounds} "
                  f"rounds)  {bw / 1e12:5.2f} TB/s of {traffic[k] / 1e6:.1f} MB = {100 * bw / HBM_PEAK:4.1f} % of peak  "
                  f"x{med[k] / base:.2f} of rope", flush=True)


def step_mode(a):
    from distributed_training_compare_jax_amd.config.schema import (ModelConfig, OptimConfig, TrainConfig, load_yaml,
                                                                     model_config_from_preset, replace)
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine

    dev = torch.device("cuda", 0)
    if a.model == "1p3b":
        base = ModelConfig(vocab_size=50258, **load_yaml(os.path.join(ROOT, "configs",
                                                                      "model_config_gpt_1p3b_gqa_rope_rms_swiglu.yaml")))
        batch = 4
    else:
        base, batch = model_config_from_preset(a.model, pos_emb="rope"), 8

    def run(qk):
        mc = replace(base, qk_norm=qk)
        tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=a.steps + a.warmup, log_every=10 ** 9,
                         output_dir="/tmp/qknorm_ab", use_graph=True)
        eng = Engine(mc, tc, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl"))
        data = get_batch_iterator(batch, mc.max_seq_len + 1, seed=0)
        t0 = 0.0
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            eng.set_batch(next(data))
            eng.run_step()
            loss = eng.loss_value()  # blocking read of this step's loss, as bench.py
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        eng.close()
        del eng
        torch.cuda.empty_cache()
        return ms, loss

    res = {"none": [], "rmsnorm": []}
    for r in range(a.rounds):
        for qk in res:
            ms, loss = run(qk)
            res[qk].append(ms)
            print(f"round {r} qk_norm {qk:8s} {ms:8.3f} ms/step over {a.steps} steps (last loss {loss:.4f})", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"qk_norm {k:8s} median {med[k]:.3f} ms/step, spread {min(v):.3f} .. {max(v):.3f}")
    d = med["rmsnorm"] - med["none"]
    print(f"{a.model}: rmsnorm - none = {d * 1e3:.1f} us/step = {d * 1e3 / base.n_layers:.2f} us per layer "
          f"({100 * d / med['none']:.2f} % of the step)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    a.rounds = a.rounds or (3 if a.step else 7)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    step_mode(a) if a.step else kernel_mode(a)
