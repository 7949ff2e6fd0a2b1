"""The local passes of ``zero_comm: p2p`` (parallel/p2p.py P2PZeroShard) per call at GPT-2 small bucket sizes, next to
what they replace, with W ranks:

* the bucket reduce-scatter (pack, barrier, reduce of the own slice into the grads + its sum of squares) against the
  bucket all-reduce of ``dp_comm: p2p`` (pack, barrier, reduce, barrier, gather), both payloads, at the production
  grid cap;
* the parameter gather with the fused bf16 mirror write against an all-gather of the same fp32 shards (the P2P
  ``all_gather`` call) followed by the full-bucket ``cast_to_bf16`` that ``refresh_mirror`` runs.

On a multi-GPU node these would be xGMI numbers; with the W processes on ONE device (or W = 1: the rehearsal's world)
they price the kernel path itself -- launches, device barriers, the passes at HBM speed -- not link bandwidth.

    python benchmarks/zero_p2p_bench.py [--world 2] [--reps 20] [--mb 40,16] [--json out.json]

Every variant is captured and timed twice and the faster pass kept (see the comment at the loop).
"""

import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# MB of fp32 gradients: dp_bucket_mb = 40 (the bulk buckets) and dp_tail_mb = 16 (the last one)
SIZES_MB = "40,16"


def _worker(reps, mb, out_dir):
    SIZES = [(int(x) << 20) // 4 for x in mb.split(",")]  # elements, divisible by 8 W
    os.environ.setdefault("DTC_DIST_BACKEND", "gloo")
    os.environ.setdefault("DTC_WORLD1_PG", "1")
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.ops.optim import cast_to_bf16
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.parallel.p2p import P2PZeroShard

    d = init_distributed("cuda")
    W = d.world
    ar = P2PZeroShard(dist.group.WORLD, d.rank, W, d.device, [(0, max(SIZES))], "fp32", use_stream=False)
    res = {}
    for n in SIZES:
        g = torch.randn(n, device=d.device)
        p = torch.randn(n, device=d.device)
        mirror = torch.empty(n, dtype=torch.bfloat16, device=d.device)
        shard = p[d.rank * (n // W):(d.rank + 1) * (n // W)].clone()
        parts = {bf: torch.zeros(ar.rs_slots(n, bf), device=d.device) for bf in (False, True)}

        def ag_cast():
            ar.all_gather(shard, p)
            cast_to_bf16(p, mirror)

        variants = [("all-reduce fp32", lambda: ar.bucket_all_reduce_(g, bf16=False)),
                    ("reduce-scatter fp32", lambda: ar.bucket_reduce_scatter_(g, parts[False], bf16=False)),
                    ("all-reduce bf16", lambda: ar.bucket_all_reduce_(g, bf16=True)),
                    ("reduce-scatter bf16", lambda: ar.bucket_reduce_scatter_(g, parts[True], bf16=True)),
                    ("all-gather + cast", ag_cast),
                    ("param gather + mirror", lambda: ar.bucket_param_gather_(p, mirror, n, bf16=False))]
        # two passes over the variants, the faster one kept: with W = 2 processes on one GPU the SECOND graph a
        # process captures replays slow whatever it holds (all-reduce or reduce-scatter, 16 to 40 MB: 1.8 to 2.5 x),
        # in all three replays; not explained, and a property of this rig, not of a kernel
        for name, call in variants + variants:
            # captured: reps calls in one hipGraph (how the step runs them), timed by events
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                gr.capture_begin(capture_error_mode="thread_local")
                for _ in range(reps):
                    call()
                ar.end_step()
                gr.capture_end()
            torch.cuda.current_stream().wait_stream(s)
            times = []
            for _ in range(3):
                g.normal_()  # (the in-place sums would grow without bound)
                torch.cuda.synchronize()
                dist.barrier()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / reps)
            ar.check()
            key = f"{name} {n * 4 >> 20} MB"
            res[key] = min(times + [res.get(key, float("inf"))])
            del gr
    torch.save(res, os.path.join(out_dir, f"r{d.rank}.pt"))
    ar.close()
    destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mb", default=SIZES_MB, help="bucket sizes in MB of fp32 gradients, comma-separated")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from distributed_training_compare_jax_amd.parallel.dist import spawn

    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, a.world, args=(a.reps, a.mb, td))
        r = [torch.load(os.path.join(td, f"r{i}.pt")) for i in range(a.world)]
    ndev = torch.cuda.device_count()
    print(f"ZeRO-1 P2P passes, W={a.world} ranks on {min(ndev, a.world)} device(s): us per call (captured, min of 2 x 3)")
    out = {}
    for k in r[0]:
        v = max(x[k] for x in r)
        out[k] = v
        print(f"  {k:32s} {v:9.1f} us")
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
