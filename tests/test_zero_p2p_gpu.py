"""The in-graph ZeRO-1 transport (``csrc/p2p.hip`` dtc_dp_reduce_scatter / dtc_dp_param_gather,
``parallel.p2p.P2PZeroShard``) bit for bit, on the rig of tests/test_dp_p2p_gpu.py: one spawned test per world W in
{2, 3, 5, 8}, W processes on one GPU over gloo, that file's input generator, sizes, sentinel guards and emulations.

* reduce-scatter, both payloads: ``grads[own slice]`` equals ``emu_bucket`` (what the all-reduce leaves there),
  compared with ``!=``; every element outside the slice keeps the bits it held (the rank's own input) and the guard
  behind ``n`` its sentinel.  The per-block partials sum (in float64) to the float64 sum of squares of the expected
  slice within a bound from the accumulation depth (:func:`sumsq_bound`); an empty slice gives exactly 0.
* parameter gather: ``params`` equals the concatenation of the ranks' owned slices (every rank's buffer holds
  different values everywhere, so a slice from the wrong rank shows), ``mirror[:n_mirror]`` equals
  ``cast_to_bf16(params)[:n_mirror]`` with ``n_mirror`` inside the bucket, at its edge, past it and before it; the
  guards behind ``n`` and ``n_mirror`` stay.
* the call sequence -- five reduce-scatters, the 4-float sum, five gathers, ``end_step`` -- eagerly without a host
  sync, then as one hipGraph replayed three times on fresh inputs (a half-alternation error shows here).
* the host validation raises through ``N.check`` and launches nothing.  No case provokes a barrier timeout.
"""

import json
import os
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

from test_dp_p2p_gpu import GUARD, N_BIG, SENT, WORLDS, _Ctx, _EndStep, _Loss, emu_bucket, inputs, sizes, slice_bounds

BF16, F32 = torch.bfloat16, torch.float32
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ emulations
# (csrc/p2p.hip, "ZeRO-1 over the DP buckets"), written from the header's formulas and from no kernel output

def owned(a, b, world, rank, bf16):
    """Elements of bucket [a, b) that ``rank`` owns: pieces of 4 (fp32 payload) or 8 (bf16) elements."""
    n, e = b - a, 8 if bf16 else 4
    lo, hi = slice_bounds(-(-n // e), world, rank)
    return a + min(n, e * lo), a + min(n, e * hi)


def emu_scatter(xs, rank, bf16):
    """What rank ``rank`` holds after the reduce-scatter: the all-reduce's values in its slice, its input elsewhere."""
    n = xs[0].numel()
    lo, hi = owned(0, n, len(xs), rank, bf16)
    out = xs[rank].clone()
    out[lo:hi] = emu_bucket(xs, bf16)[lo:hi]
    return out


def emu_gather(ps, bf16):
    """Every rank's parameters after the gather: each element from its owner's buffer."""
    n = ps[0].numel()
    out = torch.empty(n, dtype=F32)
    for r in range(len(ps)):
        lo, hi = owned(0, n, len(ps), r, bf16)
        out[lo:hi] = ps[r][lo:hi]
    return out


def emu_mirror(p, n_mirror):
    return p[:n_mirror].to(BF16)  # round-to-nearest-even, what cast_to_bf16 does


def sumsq_bound(depth):
    """Relative error bound of the fp32 sum of squares whose longest chain of additions is ``depth`` fused
    multiply-adds in one thread (each rounds once), then 6 wave shuffles and 3 adds across the 4 waves; the partials
    are summed in float64.  All terms are positive: gamma_d = d u / (1 - d u)."""
    d = (depth + 9) * U24
    return d / (1 - d)


def thread_depth(n, bf16, world, blocks):
    """Fused multiply-adds of the busiest thread: its visits to the largest slice times the elements per piece."""
    e = 8 if bf16 else 4
    chunk = -(-(-(-n // e)) // world)
    return -(-chunk // (blocks * 256)) * e


# ------------------------------------------------------------------------------------------------ worker side

def _bits(p, m):
    return torch.cat([p.cpu().view(torch.int32), m.cpu().view(torch.int16).to(torch.int32)])


class _Scatter:
    def __init__(self, c, n, bf16, max_blocks):
        self.c, self.n, self.bf16, self.mb = c, n, bf16, max_blocks
        self.name = f"scatter[n={n},{'bf16' if bf16 else 'f32'},blocks={max_blocks}]"
        self.slots = c.ar.rs_slots(n, bf16, max_blocks)
        self.b = torch.full((n + GUARD,), SENT, dtype=F32, device=c.dev)
        self.part = torch.full((self.slots + GUARD,), SENT, dtype=F32, device=c.dev)

    def load(self, key):
        xs = inputs((key, self.name), self.n, self.c.world)
        self.b.fill_(SENT)
        self.part.fill_(SENT)
        self.b[:self.n].copy_(xs[self.c.rank])
        self.exp = torch.cat([emu_scatter(xs, self.c.rank, self.bf16), torch.full((GUARD,), SENT)])
        lo, hi = owned(0, self.n, self.c.world, self.c.rank, self.bf16)
        self.empty = hi == lo
        self.ref_sq = float((self.exp[lo:hi].double() ** 2).sum())

    def issue(self):
        self.c.ar.bucket_reduce_scatter_(self.b[:self.n], self.part[:self.slots], bf16=self.bf16, max_blocks=self.mb)

    def result(self):
        return self.b.cpu()

    def extra(self, case):
        part = self.part.cpu()
        self.c.record(f"{case}/part_guard", bool((part[self.slots:] == SENT).all()))
        got = float(part[:self.slots].double().sum())
        if self.empty:
            self.c.record(f"{case}/sumsq_empty", bool((part[:self.slots] == 0).all()), note=str(got))
            return
        bound = sumsq_bound(thread_depth(self.n, self.bf16, self.c.world, self.slots))
        err = abs(got - self.ref_sq) / self.ref_sq
        print(f"ZERO-SUMSQ | {case} | rank {self.c.rank} | err {err:.3e} | bound {bound:.3e}")
        self.c.record(f"{case}/sumsq", err <= bound, note=f"err {err:.3e} bound {bound:.3e}")


class _PGather:
    """``nm``: the mirror's length as the engine counts it, relative to the bucket's start (clamped like
    P2PShardedAdamW.step does); <= 0: the bucket lies behind the mirror."""

    def __init__(self, c, n, bf16, nm):
        self.c, self.n, self.bf16 = c, n, bf16
        self.k = min(max(nm, 0), n)
        self.name = f"gather[n={n},{'bf16' if bf16 else 'f32'},mirror={nm}]"
        self.p = torch.full((n + GUARD,), SENT, dtype=F32, device=c.dev)
        self.m = torch.full((n + GUARD,), SENT, dtype=BF16, device=c.dev)

    def load(self, key):
        ps = inputs((key, self.name), self.n, self.c.world)
        self.p.fill_(SENT)
        self.m.fill_(SENT)
        self.p[:self.n].copy_(ps[self.c.rank])
        full = emu_gather(ps, self.bf16)
        self.exp = _bits(torch.cat([full, torch.full((GUARD,), SENT)]),
                         torch.cat([emu_mirror(full, self.k), torch.full((self.n + GUARD - self.k,), SENT, dtype=BF16)]))

    def issue(self):
        self.c.ar.bucket_param_gather_(self.p[:self.n], self.m if self.k else None, self.k, bf16=self.bf16)

    def result(self):
        return _bits(self.p, self.m)


def _verify(c, name, ops):
    torch.cuda.synchronize()
    for i, op in enumerate(ops):
        got = op.result()
        if got is None:
            continue
        assert got.shape == op.exp.shape and got.dtype == op.exp.dtype
        ne = (got != op.exp).reshape(-1)
        nd = int(ne.sum())
        c.record(f"{name}/{i}:{op.name}", nd == 0, nd, int(ne.nonzero()[0]) if nd else -1)
        if hasattr(op, "extra"):
            op.extra(f"{name}/{i}")
    c.ar.check()  # no barrier timed out, host and device agree on the buffer half
    c.record(f"{name}/check", True)


def _run(c, name, ops, key="eager"):
    for i, op in enumerate(ops):
        op.load((name, i, key))
    for op in ops:
        op.issue()   # no host sync in between
    _verify(c, name, ops)


def _sequence(c):
    """Five reduce-scatters, the 4-float sum, five gathers on the same buckets, end_step: 11 calls (odd), so every
    buffer half is reused and the padding round runs; both payloads and a capped grid in between."""
    W = c.world
    bk = [(8 * W + 4, True, None), (4 * 1031, False, None), (40004, True, 1), (8, False, None), (8 * 1031, True, 2)]
    nm = [8 * W + 4, 2048, 40004 + 64, 0, 4 * 1031]
    return ([_Scatter(c, n, bf, mb) for n, bf, mb in bk] + [_Loss(c)]
            + [_PGather(c, n, bf, k) for (n, bf, _), k in zip(bk, nm)] + [_EndStep(c)])


def _raises(fn):
    try:
        fn()
    except RuntimeError as e:
        return "4001" in str(e)
    return False


def _validation(c):
    from distributed_training_compare_jax_amd.ops import _native as N

    ar = c.ar
    L, st = N.lib(), N.stream_ptr(c.dev)
    x = torch.zeros(64, device=c.dev)
    m = torch.zeros(64, dtype=BF16, device=c.dev)
    part = torch.zeros(8, device=c.dev)
    big = torch.empty(ar.half // 4 + 4, device=c.dev)
    huge = torch.empty(c.world * (ar.half // 4) + 8 * c.world, device=c.dev)  # rank 0's slice exceeds the half
    calls, epoch = ar.calls, int(ar.epoch.item())
    # through the binding: N.check raises on the file's 4001
    c.record("validation/rs n%4", _raises(lambda: ar.bucket_reduce_scatter_(x[:6], part[:1])))
    c.record("validation/rs oversize", _raises(lambda: ar.bucket_reduce_scatter_(big, part[:1], bf16=False)))
    c.record("validation/ag n%4", _raises(lambda: ar.bucket_param_gather_(x[:6], m, 4)))
    c.record("validation/ag oversize", _raises(lambda: ar.bucket_param_gather_(huge, None, 0, bf16=False)))
    rs = lambda p, n, bf, pt, ns, mb: L.dtc_dp_reduce_scatter(p, n, bf, pt, ns, ar._bases_ptr, c.rank, c.world,  # noqa: E731
                                                              ar.half, ar.epoch.data_ptr(), ar.err.data_ptr(), mb, st)
    ag = lambda p, mi, n, nm, mb: L.dtc_dp_param_gather(p, mi, n, nm, 0, ar._bases_ptr, c.rank, c.world,  # noqa: E731
                                                        ar.half, ar.epoch.data_ptr(), ar.err.data_ptr(), mb, st)
    bad = {"rs misaligned": rs(x.data_ptr() + 4, 8, 0, part.data_ptr(), 1, 64),
           "rs blocks<1": rs(x.data_ptr(), 8, 0, part.data_ptr(), 1, 0),
           "rs blocks>1024": rs(x.data_ptr(), 8, 0, part.data_ptr(), 1, 1025),
           "rs slots": rs(x.data_ptr(), 8, 0, part.data_ptr(), 2, 64),
           "rs null": rs(0, 8, 0, part.data_ptr(), 1, 64),
           "ag misaligned": ag(x.data_ptr() + 4, m.data_ptr(), 8, 8, 1024),
           "ag mirror>n": ag(x.data_ptr(), m.data_ptr(), 8, 12, 1024),
           "ag mirror%4": ag(x.data_ptr(), m.data_ptr(), 8, 6, 1024),
           "ag no mirror": ag(x.data_ptr(), 0, 8, 8, 1024),
           "ag blocks<1": ag(x.data_ptr(), m.data_ptr(), 8, 8, 0),
           "ag blocks>1024": ag(x.data_ptr(), m.data_ptr(), 8, 8, 1025)}
    torch.cuda.synchronize()
    for k, rc in bad.items():
        c.record(f"validation/{k}", rc == 4001, note=str(rc))
    c.record("validation/nothing_ran", ar.calls == calls and int(ar.epoch.item()) == epoch)


def _worker(out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.parallel.p2p import DP_P2P_BLOCKS, P2PZeroShard, zero_half_bytes

    d = init_distributed("cuda")
    W = d.world
    torch.set_num_threads(max(1, 8 // W))
    bks = [(0, N_BIG), (N_BIG, N_BIG + 40004)]
    ar = P2PZeroShard(dist.group.WORLD, d.rank, W, d.device, bks, "fp32", use_stream=False)
    assert ar.half == zero_half_bytes(bks, W, "fp32") == (N_BIG * 4 + 4095) // 4096 * 4096
    assert ar.max_blocks == DP_P2P_BLOCKS
    c = _Ctx(ar, d, os.path.join(out_dir, f"rank{d.rank}.json"))
    for n, mb in sizes(W):
        for bf in (False, True):
            # two calls on different inputs: both buffer halves at every size
            _run(c, f"size{n}_{'bf16' if bf else 'f32'}", [_Scatter(c, n, bf, mb), _Scatter(c, n, bf, mb)])
            inside = max(4, n // 8 * 4)
            _run(c, f"gsize{n}_{'bf16' if bf else 'f32'}",
                 [_PGather(c, n, bf, inside), _PGather(c, n, bf, n), _PGather(c, n, bf, n + 64), _PGather(c, n, bf, -64)])
    _run(c, "production_cap", [_Scatter(c, N_BIG, False, None), _Scatter(c, N_BIG, True, None),
                               _PGather(c, N_BIG, False, N_BIG // 8 * 4), _PGather(c, N_BIG, True, N_BIG)])
    assert ar.calls % 2 == 0
    ops = _sequence(c)
    _run(c, "sequence", ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="thread_local")
        for op in ops:
            op.issue()
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    for r in range(3):
        for i, op in enumerate(ops):
            op.load(("sequence_graph", i, r))   # fresh inputs into the static buffers
        g.replay()
        _verify(c, f"sequence_graph/replay{r}", ops)
    _validation(c)
    c.flush()
    ar.close()
    destroy()


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("world", WORLDS)
def test_zero_reduce_scatter_and_param_gather_bitwise(cuda, world):
    err = None
    with tempfile.TemporaryDirectory() as td:
        try:
            spawn(_worker, world, args=(td,))
        except Exception as e:  # a worker raised at its first mismatch: show what the reports hold
            err = e
        reps = []
        for r in range(world):
            p = os.path.join(td, f"rank{r}.json")
            reps.append(json.load(open(p)) if os.path.exists(p) else None)
    bad = [(r, e) for r, rep in enumerate(reps) if rep for e in rep if not e["ok"]]
    assert err is None and not bad, f"world {world}: {bad[:8]} {err}"
    assert all(rep for rep in reps)
    names = [e["case"] for e in reps[0]]
    assert len(names) == len(set(names))
    bitwise = [n for n in names if ":" in n or n.endswith("/check") or n.startswith("validation/")]
    for rep in reps:  # the Σg² entries differ by rank (sumsq / sumsq_empty); everything else is the same list
        assert [e["case"] for e in rep if e["case"] in set(bitwise)] == bitwise
    # every size in both payloads twice, four mirror lengths per size and payload, the production cap, the sequence
    # eagerly and in 3 replays, the refusals
    assert sum(n.startswith("size") and ":scatter" in n for n in names) == 4 * len(sizes(world))
    assert sum(n.startswith("gsize") and ":gather" in n for n in names) == 8 * len(sizes(world))
    assert sum(n.startswith("production_cap/") and (":scatter" in n or ":gather" in n) for n in names) == 4
    for rep in reps:
        cases = [e["case"] for e in rep]
        assert sum(x.endswith("/sumsq") or x.endswith("/sumsq_empty") for x in cases) == \
            sum(":scatter" in x for x in cases)
    # n = 4 with the bf16 payload: one piece, every rank but the first owns nothing and reports exact zeros
    assert all(any(e["case"].startswith("size4_bf16/") and e["case"].endswith("/sumsq_empty") for e in rep)
               for rep in reps[1:])
    for what in ["sequence"] + [f"sequence_graph/replay{r}" for r in range(3)]:
        got = [n for n in names if n.startswith(what + "/")]
        assert sum(":scatter" in n for n in got) == 5 and sum(":gather" in n for n in got) == 5
        assert any(n.endswith(":loss_sum") for n in got) and any(n.endswith("/check") for n in got)
    assert sum(n.startswith("validation/") for n in names) == 16
