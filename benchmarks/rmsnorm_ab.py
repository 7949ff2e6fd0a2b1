"""The RMSNorm kernels (csrc/rmsnorm.hip) against the LayerNorm kernels (csrc/norm_reduce.hip) at the same (M, D),
HBM-cold, and the gpt-1.3b step with ``norm: rmsnorm`` against ``layernorm``.

    python benchmarks/rmsnorm_ab.py [--rounds 7] [--reps 8]      # kernels: forward (residual-add form) and backward
    python benchmarks/rmsnorm_ab.py --step [--steps 20] [--warmup 5] [--rounds 3] [--preset gpt-1.3b] [--batch 8]

Kernel mode.  Shapes: gpt2-small (8192 tokens, D 768) and gpt-1.3b (16384 tokens, D 2048).  The forward is the form
the default step runs, ``x = float(d) + resid`` with a bf16 ``d``, fp32 ``x`` out, bf16 ``y``; the backward is the
block's, bf16 ``dy``, ``dres``, a bf16 copy of ``dx`` and the fused bias-gradient slab, with the direct slab reduction.
Cold operands by rotation: ``reps`` sets of operands (more than 600 MB together, past the 256 MB last-level cache) are
visited in turn inside one captured graph; the time is the replay's device-event time over ``reps``.  The two norms
alternate in the same process.  Reported: median, min and max over the rounds, the minimal traffic and its rate, and
the ratio RMSNorm / LayerNorm.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_compare_jax_amd.ops import layernorm as LN  # noqa: E402
from distributed_training_compare_jax_amd.ops import rmsnorm as RN  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
SHAPES = {"gpt2-small": (8192, 768), "gpt-1.3b": (16384, 2048)}  # M, D
EPS = 1e-6


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
    bf, f32 = torch.bfloat16, torch.float32
    for name, (M, D) in SHAPES.items():
        reps = max(a.reps, -(-600 * 2 ** 20 // (M * D * 14)))
        g, b = torch.randn(D, device=dev), torch.randn(D, device=dev)
        dg, db, dbias = (torch.zeros(D, device=dev) for _ in range(3))
        sets = [dict(d=torch.randn(M, D, device=dev).to(bf), x=5.0 + torch.randn(M, D, device=dev),
                     dy=torch.randn(M, D, device=dev).to(bf), dres=torch.randn(M, D, device=dev),
                     dxc=torch.empty(M, D, dtype=bf, device=dev)) for _ in range(reps)]
        for s in sets:
            s["mu"], s["rs"] = s["x"].mean(-1), torch.rsqrt(s["x"].var(-1, unbiased=False) + EPS)
            s["rrs"] = torch.rsqrt(s["x"].pow(2).mean(-1) + EPS)
        runs = {
            "ln  fwd": [lambda s=s: LN.add_layernorm_fwd(s["d"], s["x"], g, b, EPS, bf) for s in sets],
            "rms fwd": [lambda s=s: RN.add_rmsnorm_fwd(s["d"], s["x"], g, EPS, bf) for s in sets],
            "ln  bwd": [lambda s=s: LN.layernorm_bwd(s["dy"], s["x"], g, s["mu"], s["rs"], s["dres"], dg, db, 0.0,
                                                     out=s["dres"], out_c=s["dxc"], dbias=dbias) for s in sets],
            "rms bwd": [lambda s=s: RN.rmsnorm_bwd(s["dy"], s["x"], g, s["rrs"], s["dres"], dg, 0.0, out=s["dres"],
                                                   out_c=s["dxc"], dbias=dbias) for s in sets]}
        for f in runs.values():
            f[0]()
        torch.cuda.synchronize()
        res = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, f in runs.items():
                res[k].append(graph_time(f))
        # minimal traffic: fwd d 2 + resid 4 + x 4 + y 2; bwd dy 2 + x 4 + dres 4 + dx 4 + dx_c 2 bytes per element
        nbytes = {"fwd": M * D * 12, "bwd": M * D * 16}
        med = {k: statistics.median(v) for k, v in res.items()}
        for k, v in res.items():
            bw = nbytes[k[4:]] / (med[k] * 1e-6)
            print(f"{name:10s} M {M} D {D} {k} {med[k]:7.1f} us (min {min(v):.1f} max {max(v):.1f}, {reps} sets, "
                  f"{a.rounds} rounds)  {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of peak  "
                  f"x{med[k] / med['ln  ' + k[4:]]:.3f} of LayerNorm", flush=True)


def step_mode(a):
    from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
    from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine

    dev = torch.device("cuda", 0)

    def run(norm):
        mc = model_config_from_preset(a.preset, norm=norm)
        tc = TrainConfig(seed=0, parallel="dp", batch=a.batch, steps=a.steps + a.warmup, log_every=10 ** 9,
                         output_dir="/tmp/rmsnorm_ab", use_graph=True)
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
        return ms, loss

    res = {"layernorm": [], "rmsnorm": []}
    for r in range(a.rounds):
        for norm in res:
            ms, loss = run(norm)
            res[norm].append(ms)
            print(f"round {r} {a.preset} {norm:9s} {ms:8.3f} ms/step over {a.steps} steps (last loss {loss:.4f})", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"{k:9s} median {med[k]:.3f} ms/step, spread {min(v):.3f} .. {max(v):.3f}")
    print(f"rmsnorm - layernorm = {(med['rmsnorm'] - med['layernorm']) * 1e3:.1f} us/step")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preset", default="gpt-1.3b")
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    a.rounds = a.rounds or (3 if a.step else 7)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    step_mode(a) if a.step else kernel_mode(a)
