"""The RoPE kernel (csrc/rope.hip) against a device-to-device copy of the same bytes, HBM-cold, and the gpt2-small
step with ``pos_emb: rope`` against ``learned``.

    python benchmarks/rope_ab.py [--rounds 7] [--reps 16]      # kernel: forward and inverse at two shapes
    python benchmarks/rope_ab.py --step [--steps 60] [--warmup 10] [--rounds 3]

Kernel mode.  Shapes: gpt2-small (8192 tokens, H 12, hd 64) and gpt-1.3b-gqa (8 x 2048 tokens, H 16, Hkv 4, hd 128),
bf16.  Cold operands by rotation: ``reps`` copies of the activation (more than 600 MB together, past the 256 MB last-
level cache) are visited in turn inside one captured graph, so every call reads its tensor from HBM; the time is the
replay's device-event time over ``reps``.  The yardstick, alternating with the kernel in the same process, is
``torch`` copying the same rotated columns between two such sets (the same minimal traffic: every byte read once and
written once).  Reported: the median time, bytes/s against the minimal traffic ``2 * rows * (H + Hkv) * hd *
sizeof(T)``, the ratio to the copy, and the share of the 8 TB/s HBM peak.

Step mode.  ``bench.py --set`` reaches ``TrainConfig`` only, so this runs ``bench.py``'s engine loop at its gpt2-small
setting (8 sequences, one GPU, hipGraph) with ``pos_emb`` learned and rope, alternating, ``steps`` timed steps after
``warmup`` per run, and prints each run's ms/step, the spread of each variant and the difference per step: the cost of
the 24 extra launches (one per layer and direction), which a fusion into the qkv epilogue or the attention loads would
have to beat.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
        ld, nrot = (H + 2 * Hkv) * hd, (H + Hkv) * hd
        reps = max(a.reps, -(-600 * 2 ** 20 // (B * T * ld * 2)))
        xs = [torch.randn(B, T, ld, device=dev).to(torch.bfloat16) for _ in range(reps)]
        ys = [torch.empty_like(x) for x in xs]
        tab = rope_table(T, hd, 10000.0, dev)
        runs = {"fwd": [lambda x=x: rope_(x, tab, H, Hkv) for x in xs],
                "inv": [lambda x=x: rope_(x, tab, H, Hkv, inverse=True) for x in xs],
                "copy": [lambda x=x, y=y: y[..., :nrot].copy_(x[..., :nrot]) for x, y in zip(xs, ys)]}
        for f in runs.values():
            f[0]()
        torch.cuda.synchronize()
        res = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, f in runs.items():
                res[k].append(graph_time(f))
        nbytes = 2 * B * T * nrot * 2
        med = {k: statistics.median(v) for k, v in res.items()}
        for k, v in res.items():
            bw = nbytes / (med[k] * 1e-6)
            print(f"{name:13s} {k:4s} {med[k]:7.1f} us (min {min(v):.1f} max {max(v):.1f}, {reps} tensors, {a.rounds} "
                  f"rounds)  {bw / 1e12:5.2f} TB/s of {nbytes / 1e6:.1f} MB = {100 * bw / HBM_PEAK:4.1f} % of peak  "
                  f"x{med[k] / med['copy']:.2f} of the copy", flush=True)


def step_mode(a):
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine

    dev = torch.device("cuda", 0)

    def run(pos):
        mc = model_config_from_preset("gpt2-small", pos_emb=pos)
        tc = TrainConfig(seed=0, parallel="dp", batch=8, steps=a.steps + a.warmup, log_every=10 ** 9,
                         output_dir="/tmp/rope_ab", use_graph=True)
        eng = Engine(mc, tc, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl"))
        data = get_batch_iterator(8, mc.max_seq_len + 1, seed=0)
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
        return ms, loss

    res = {"learned": [], "rope": []}
    for r in range(a.rounds):
        for pos in res:
            ms, loss = run(pos)
            res[pos].append(ms)
            print(f"round {r} {pos:8s} {ms:8.3f} ms/step over {a.steps} steps (last loss {loss:.4f})", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"{k:8s} median {med[k]:.3f} ms/step, spread {min(v):.3f} .. {max(v):.3f}")
    d = med["rope"] - med["learned"]
    n = 2 * 12  # one launch per layer and direction: the Q and K heads are one contiguous range of columns
    print(f"rope - learned = {d * 1e3:.1f} us/step = {d * 1e3 / n:.2f} us per extra launch ({n} launches)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    a.rounds = a.rounds or (3 if a.step else 7)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    step_mode(a) if a.step else kernel_mode(a)
