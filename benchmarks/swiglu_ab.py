"""The fused SwiGLU kernels (csrc/swiglu.hip glu_fwd_kernel / glu_bwd_kernel) against the unfused path (an ordinary GEMM
with an fp32 output + an elementwise kernel), HBM-cold, and the step of a ``mlp: swiglu`` model at either shape fused against unfused.

    python benchmarks/swiglu_ab.py [--shape gpt2-small|gpt-1.3b] [--rounds 5] [--reps 4]
    python benchmarks/swiglu_ab.py --step [--shape ...] [--steps 10] [--warmup 3] [--rounds 3] [--batch 8]

Kernel mode.  Shapes (M, D, F): gpt2-small-like (8192, 768, 2048) and the swiglu preset's (16384, 2048, 5632).  Forward:
``swiglu_fc1`` (gu and h from x, fc1.w, fc1.b); backward: ``swiglu_fc2_dgrad`` on the transposed fc2 mirror.  For scale
the existing GELU pair (``linear_gelu``, N = F, two bf16 outputs) runs at the same (M, D, F).  Cold operands by rotation:
``reps`` sets of activations (more than 600 MB together, past the 256 MB last-level cache) are visited in turn inside one
captured graph; the time is the replay's device-event time over ``reps``.  The variants alternate in the same process.
Reported: median, min and max over the rounds and the rate over the GEMM's FLOPs (2 M D 2F forward, 2 M D F backward and
GELU pair).  One invocation does one shape or the step, so a caller can put each under a time limit of its own.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_compare_jax_amd.ops import gemm as G  # noqa: E402
from distributed_training_compare_jax_amd.ops import swiglu as SW  # noqa: E402

SHAPES = {"gpt2-small": (8192, 768, 2048), "gpt-1.3b": (16384, 2048, 5632)}  # M, D, F


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


def with_knob(v, f):
    def run():
        os.environ["DTC_SWIGLU_FUSE"] = v
        f()
    return run


def kernel_mode(a):
    dev, bf = torch.device("cuda"), torch.bfloat16
    M, D, F = SHAPES[a.shape]
    reps = max(a.reps, -(-600 * 2 ** 20 // (M * (2 * D + 5 * F) * 2)))
    w = (0.05 * torch.randn(2 * F, D, device=dev)).to(bf)
    b = torch.randn(2 * F, device=dev)
    w2 = (0.05 * torch.randn(D, F, device=dev)).to(bf)
    w2t = w2.t().contiguous()
    sets = [dict(x=torch.randn(M, D, device=dev).to(bf), dy=torch.randn(M, D, device=dev).to(bf),
                 gu=torch.randn(M, 2 * F, device=dev).to(bf)) for _ in range(reps)]
    runs = {"fwd fused": [with_knob("2", lambda s=s: SW.swiglu_fc1(s["x"], w, b)) for s in sets],
            "fwd unfused": [with_knob("0", lambda s=s: SW.swiglu_fc1(s["x"], w, b)) for s in sets],
            "fwd gelu pair": [lambda s=s: G.linear_gelu(s["x"], w[:F], b[:F]) for s in sets],
            "bwd fused": [with_knob("2", lambda s=s: SW.swiglu_fc2_dgrad(s["dy"], w2, w2t, s["gu"])) for s in sets],
            "bwd unfused": [with_knob("0", lambda s=s: SW.swiglu_fc2_dgrad(s["dy"], w2, w2t, s["gu"])) for s in sets]}
    for k, f in runs.items():
        f[0]()
        if k.endswith("fused"):
            want = "unfused" if "unfused" in k else "fused"
            assert SW.LAST["fc1" if k.startswith("fwd") else "fc2_dgrad"] == want, (k, SW.LAST)
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, f in runs.items():
            res[k].append(graph_time(f))
    flops = {"fwd fused": 4.0 * M * D * F, "fwd unfused": 4.0 * M * D * F}
    for k, v in res.items():
        med = statistics.median(v)
        tf = flops.get(k, 2.0 * M * D * F) / (med * 1e-6) / 1e12
        print(f"{a.shape:10s} M {M} D {D} F {F} {k:13s} {med:8.1f} us (min {min(v):.1f} max {max(v):.1f}, {reps} sets, "
              f"{a.rounds} rounds)  {tf:6.1f} TF/s", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print(f"{a.shape}: fused / unfused  fwd x{med['fwd fused'] / med['fwd unfused']:.3f}  "
          f"bwd x{med['bwd fused'] / med['bwd unfused']:.3f}")


def step_mode(a):
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine

    dev = torch.device("cuda", 0)

    def run(fuse):
        os.environ["DTC_SWIGLU_FUSE"] = fuse
        if a.shape == "gpt-1.3b":  # configs/model_config_gpt_1p3b_gqa_rope_rms_swiglu.yaml
            mc = model_config_from_preset("gpt-1.3b", n_kv_heads=4, pos_emb="rope", norm="rmsnorm", mlp="swiglu", d_ff=5632)
        else:
            mc = model_config_from_preset("gpt2-small", mlp="swiglu", d_ff=2048)
        tc = TrainConfig(seed=0, parallel="dp", batch=a.batch, steps=a.steps + a.warmup, log_every=10 ** 9,
                         output_dir="/tmp/swiglu_ab", use_graph=True)
        eng = Engine(mc, tc, OptimConfig(lr=3e-4, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl"))
        data = get_batch_iterator(a.batch, mc.max_seq_len + 1, seed=0)
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
        return ms, loss, dict(SW.LAST)

    res = {"2": [], "0": []}  # 2: the fused pair wherever its contract holds, 0: unfused
    for r in range(a.rounds):
        for fuse in res:
            ms, loss, last = run(fuse)
            res[fuse].append(ms)
            print(f"round {r} {a.shape} swiglu DTC_SWIGLU_FUSE={fuse} {ms:8.3f} ms/step over {a.steps} steps "
                  f"(last loss {loss:.4f}; {last})", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"DTC_SWIGLU_FUSE={k} median {med[k]:.3f} ms/step, spread {min(v):.3f} .. {max(v):.3f}")
    print(f"fused - unfused = {(med['2'] - med['0']) * 1e3:.1f} us/step")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--shape", default="gpt2-small", choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    a.rounds = a.rounds or (3 if a.step else 5)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    step_mode(a) if a.step else kernel_mode(a)
