"""In-process A/B of the document-masked attention kernels against the default unmasked ones, per layer, forward and
backward, at the GPT-2-small layer (B8 T1024 H12 hd64) and the gpt-1.3b layer at B4 (B4 T2048 H16 hd128).

    python benchmarks/attn_doc_ab.py [--rounds 5] [--reps 24] [--sets 4]

The doc kernels run with a single document and with mean document lengths 512, 256 and 64: boundaries drawn from a
seeded geometric law (every position ends a document with probability 1 / mean), the realised sum L_i^2 / T^2 (the
share of the causal work that is left) printed beside the times.  Operands are HBM-cold: every variant cycles through
``--sets`` copies of (qkv, o, lse, dO) that together exceed the 256 MB of L2 + Infinity Cache, ``reps`` calls captured
in one hipGraph and replayed; the variants are interleaved round by round and the median over rounds is reported.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_compare_jax_amd.ops import attention as A  # noqa: E402

SHAPES = [(8, 1024, 12, 64), (4, 2048, 16, 128)]
SEP = 1


def timeit(fns, reps):
    """GPU time per call: ``reps`` calls cycling through ``fns`` (one per operand set), one hipGraph, replayed."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        gr.capture_begin()
        for i in range(reps):
            fns[i % len(fns)]()
        gr.capture_end()
    torch.cuda.current_stream().wait_stream(st)
    gr.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    gr.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def geometric_ids(B, T, mean, seed):
    """ids int32 [B, T]: the separator where a seeded geometric law ends a document (mean None: nowhere)."""
    ids = np.full((B, T), SEP + 1, np.int32)
    if mean is not None:
        ids[np.random.default_rng(seed).random((B, T)) < 1.0 / mean] = SEP
    return torch.from_numpy(ids)


def work_share(doc, T):
    """(sum over documents of L^2 / T^2, averaged over rows; the realised mean document length)."""
    ds, de = doc[0].cpu().numpy(), doc[1].cpu().numpy()
    share, ndocs = [], 0
    for b in range(ds.shape[0]):
        starts = np.unique(ds[b])
        ends = np.array([de[b, s] for s in starts])
        share.append(float(((ends - starts) ** 2).sum()) / T ** 2)
        ndocs += len(starts)
    return float(np.mean(share)), ds.size / ndocs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    for B, T, H, hd in SHAPES:
        g = torch.Generator().manual_seed(0)
        sets = []
        for _ in range(a.sets):
            qkv = torch.randn(B, T, 3 * H * hd, generator=g).cuda().bfloat16()
            do = torch.randn(B, T, H * hd, generator=g).cuda().bfloat16()
            sets.append((qkv, do))
        # bytes of one set: qkv and dqkv, dO and o (bf16), lse (fp32) and the backward's delta workspace (fp32)
        mb = a.sets * (2 * (3 + 1) * B * T * H * hd * 2 + 2 * B * H * T * 4) / 2 ** 20
        print(f"## B{B} T{T} H{H} hd{hd}: {a.sets} operand sets, {mb:.0f} MB touched per cycle", flush=True)
        variants = {}

        def add(name, doc):
            saved = [A.attn_fwd(qkv, H, doc=doc) for qkv, _ in sets]
            variants["fwd " + name] = [lambda qkv=qkv: A.attn_fwd(qkv, H, doc=doc) for qkv, _ in sets]
            variants["bwd " + name] = [lambda qkv=qkv, do=do, o=o, lse=lse: A.attn_bwd(qkv, o, lse, do, H, doc=doc)
                                       for (qkv, do), (o, lse) in zip(sets, saved)]

        add("default unmasked", None)
        for mean in (None, 512, 256, 64):
            doc = tuple(t.cuda() for t in A.doc_bounds(geometric_ids(B, T, mean, seed=T + (mean or 0)), SEP))
            share, mean_len = work_share(doc, T)
            name = f"doc mean {mean or T} (realised {mean_len:.0f}, work {share:.3f})"
            add(name, doc)
        res = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fns in variants.items():
                res[k].append(timeit(fns, a.reps))
        base = {}
        for k, v in res.items():
            v = sorted(v)
            med = v[len(v) // 2]
            base.setdefault(k[:3], med)  # the first fwd / bwd entry is the unmasked default
            print(f"{k:52s} median {med:8.2f} us  min {v[0]:8.2f}  max {v[-1]:8.2f}  x{med / base[k[:3]]:.3f} of default",
                  flush=True)


if __name__ == "__main__":
    main()
