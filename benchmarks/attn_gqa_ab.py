"""In-process A/B of the grouped-query attention kernels against the multi-head kernels at the same number of query
heads, per layer, forward and backward: the gpt-1.3b layer at B4 (B4 T2048 H16 hd128) with 16 (multi-head), 4 and 1
K/V heads, and the GPT-2-small layer (B8 T1024 H12 hd64) with 12 (multi-head) and 4.

    python benchmarks/attn_gqa_ab.py [--rounds 5] [--reps 24] [--sets 4]

The multi-head rows run today's default kernels (``attn_fwd`` / ``attn_bwd`` without ``n_kv_heads``); at head_dim 64,
where the default forward is the round-5 pipeline, a ``rows32`` row adds the 32-row multi-head kernels the GQA ones
share their bodies with.  ``DTC_KERNEL_LIB=<a build with -DATTN_NO_PK_F32=>`` times the GQA kernels with packed fp32
instructions; the ``bits`` printed per variant (a sum over the outputs' bit patterns) compare the two builds.  Operands are
HBM-cold and timed as in benchmarks/attn_doc_ab.py: every variant cycles through ``--sets`` copies of (qkv, o, lse,
dO) that together exceed the 256 MB of L2 + Infinity Cache, ``reps`` calls captured in one hipGraph and replayed; the
variants are interleaved round by round and the median over rounds is reported.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attn_doc_ab import timeit  # noqa: E402
from distributed_training_compare_jax_amd.ops import attention as A  # noqa: E402

SHAPES = [(4, 2048, 16, 128, (16, 4, 1)), (8, 1024, 12, 64, (12, 4))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    for B, T, H, hd, kvs in SHAPES:
        print(f"## B{B} T{T} H{H} hd{hd}: {a.sets} operand sets", flush=True)
        variants = {}
        for kv in kvs + ((("rows32",) if hd == 64 else ())):
            tag, kw = f"Hkv {kv:2d}" if kv != "rows32" else "rows32", {}
            if kv == "rows32":  # the multi-head 32-row twins, by flag
                kv, kw = H, dict(ff=A.FwdFlags.ROUND4, bf=A.BwdFlags.FORCE_MERGED)
            fwd_fn = lambda qkv, kv=kv, kw=kw: A.attn_fwd(qkv, H, n_kv_heads=kv, flags=kw.get("ff", 0))  # noqa: E731
            bwd_fn = lambda qkv, o, lse, do, kv=kv, kw=kw: A.attn_bwd(  # noqa: E731
                qkv, o, lse, do, H, n_kv_heads=kv, flags=kw.get("bf", 0))
            g = torch.Generator().manual_seed(kv)
            sets = [(torch.randn(B, T, (H + 2 * kv) * hd, generator=g).cuda().bfloat16(),
                     torch.randn(B, T, H * hd, generator=g).cuda().bfloat16()) for _ in range(a.sets)]
            saved = [fwd_fn(qkv) for qkv, _ in sets]
            fwd = A.last_launch().kernels
            variants[f"fwd {tag}"] = [lambda qkv=qkv, f=fwd_fn: f(qkv) for qkv, _ in sets]
            variants[f"bwd {tag}"] = [lambda qkv=qkv, do=do, o=o, lse=lse, f=bwd_fn: f(qkv, o, lse, do)
                                      for (qkv, do), (o, lse) in zip(sets, saved)]
            bits = sum(int(t.view(torch.int16).long().sum()) for t in (saved[0][0], variants[f"bwd {tag}"][0]()))
            # bytes of one set: qkv and dqkv, dO and o (bf16), lse (fp32) and the backward's delta workspace (fp32)
            mb = a.sets * ((2 * (H + 2 * kv) + 2 * H) * B * T * hd * 2 + 2 * B * H * T * 4) / 2 ** 20
            print(f"{tag}: {mb:.0f} MB touched per cycle; bits {bits}; {fwd + A.last_launch().kernels}", flush=True)
        res = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fns in variants.items():
                res[k].append(timeit(fns, a.reps))
        base = {}
        for k, v in res.items():
            v = sorted(v)
            med = v[len(v) // 2]
            base.setdefault(k[:3], med)  # the first fwd / bwd entry is the multi-head one
            print(f"{k:14s} median {med:8.2f} us  min {v[0]:8.2f}  max {v[-1]:8.2f}  x{med / base[k[:3]]:.3f} of multi-head",
                  flush=True)


if __name__ == "__main__":
    main()
