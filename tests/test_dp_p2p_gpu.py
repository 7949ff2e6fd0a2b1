"""The in-graph DP bucket all-reduce (``csrc/p2p.hip`` dtc_dp_allreduce, ``parallel.p2p.P2PGradReduce``) bit for bit.

One spawned test per world W in {2, 3, 5, 8}: W processes on one GPU over gloo.  The kernels only round, add and
copy, and the file header fixes the order, so a torch loop on the CPU predicts every output bit:

* fp32 payload: ``s = x[0]; s = s + x[p]`` in rank order;
* bf16 payload: ``a = 0; a += float(bf16(x[p]))`` in rank order, one rounding of ``a`` to bf16, widened exactly.

The emulations are written from those formulas and from no kernel output (self-checked without a GPU in
tests/test_dp_p2p_cpu.py).  Every worker regenerates every rank's input (``randn * 10^U(-2, 2)``, different per
rank and per call), computes what it expects and compares on the spot with ``!=``; a sentinel guard behind
``grads + n`` must stay intact.  The sizes cover one padded bf16 piece, short and empty slices, piece counts W does
not divide, blocks that loop under ``max_blocks = 1``, and 1.1 M + 4 elements at the production cap.  The call
sequence (5 bucket calls, a loss sum and an all-gather on the same object, ``end_step``) runs eagerly without a host
sync and then as one hipGraph replayed 3 times on fresh inputs.  No case provokes a barrier timeout.
"""

import functools
import json
import os
import tempfile
import zlib

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

WORLDS = (2, 3, 5, 8)
GUARD = 64
SENT = 12345.0
BF16, F32 = torch.bfloat16, torch.float32
N_BIG = 1100000 + 4
STRIDE = 7919


# ------------------------------------------------------------------------------------------------ inputs

def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=4)
def _scale(n):
    """10^U(-2, 2), fp32 [2 n]: a window [q, q + n) is the size's vector rotated by q."""
    return torch.pow(10.0, torch.rand(n, generator=_gen("scale", n)) * 4 - 2).repeat(2)


def inputs(key, n, world):
    """Every rank's fp32 input of one call: rank p takes the normal draws [p STRIDE, p STRIDE + n) of one stream
    seeded by the key, times its own rotation of the size's scale vector."""
    z = torch.randn(n + STRIDE * world, generator=_gen(key))
    out = []
    for p in range(world):
        q = STRIDE * (p + 1) % n
        out.append(z[p * STRIDE:p * STRIDE + n] * _scale(n)[q:q + n])
    return out


# ------------------------------------------------------------------------------------------------ emulations
# (csrc/p2p.hip, "DP gradient buckets": dp_pack_kernel / dp_reduce_kernel (rank_sum_f32, rank_sum_bf16) /
# dp_gather_kernel (widen_bf16x8))

def emu_bucket(xs, bf16):
    """What every rank holds after the call, fp32 [n]."""
    if not bf16:
        s = xs[0].clone()
        for x in xs[1:]:
            s = s + x
        return s
    a = torch.zeros(xs[0].numel(), dtype=F32)
    for x in xs:
        a = a + x.to(BF16).float()   # pack: one round-to-nearest-even per element
    return a.to(BF16).float()        # reduce: one rounding of the sum; gather: bits << 16


def slice_bounds(pieces, world, rank):
    """[lo, hi) of the 16-byte pieces rank ``rank`` reduces: chunk = ceil(pieces / W)."""
    chunk = -(-pieces // world)
    lo = min(pieces, rank * chunk)
    return lo, min(pieces, lo + chunk)


def sizes(W):
    """Elements: one (padded) piece, two, the first / last slice short, piece counts W does not divide in either
    payload, and a bucket every block loops over under max_blocks = 1 (n % 8 == 4 as well)."""
    return [(4, None), (8, None), (8 * W - 4, None), (8 * W + 4, None), (4 * 1031, None), (8 * 1031, None),
            (40004, 1)]


def test_sizes_reach_the_paths_they_name():
    for W in WORLDS:
        ns = [n for n, _ in sizes(W)]
        assert all(n % 4 == 0 for n in ns)
        assert slice_bounds(-(-4 // 8), W, W - 1) == (1, 1)                      # n = 4, bf16: most ranks own nothing
        assert any((n // 4) % W for n in ns) and any(-(-n // 8) % W for n in ns)  # pieces % W != 0, both payloads
        lo, hi = slice_bounds(-(-(8 * W - 4) // 8), W, W - 1)
        assert hi - lo <= 1
        # max_blocks = 1: 256 threads, 2 pieces each per pass of the reduce, 4 per pass of the copies
        for bf in (False, True):
            pieces = -(-40004 // 8) if bf else 40004 // 4
            assert all(slice_bounds(pieces, W, r)[1] - slice_bounds(pieces, W, r)[0] > 512 for r in range(W))
            assert pieces > 2 * 1024


# ------------------------------------------------------------------------------------------------ worker side

class _Bucket:
    def __init__(self, c, n, bf16, max_blocks):
        self.c, self.n, self.bf16, self.mb = c, n, bf16, max_blocks
        self.name = f"bucket[n={n},{'bf16' if bf16 else 'f32'},blocks={max_blocks}]"
        self.b = torch.full((n + GUARD,), SENT, dtype=F32, device=c.dev)

    def load(self, key):
        xs = inputs((key, self.name), self.n, self.c.world)
        self.b.fill_(SENT)
        self.b[:self.n].copy_(xs[self.c.rank])
        self.exp = torch.cat([emu_bucket(xs, self.bf16), torch.full((GUARD,), SENT)])

    def issue(self):
        self.c.ar.bucket_all_reduce_(self.b[:self.n], bf16=self.bf16, max_blocks=self.mb)

    def result(self):
        return self.b.cpu()


class _Loss:
    """The engine's loss sum: 4 floats, the last three zero, through the existing one-shot all_reduce_."""
    name = "loss_sum"

    def __init__(self, c):
        self.c = c
        self.b = torch.zeros(4 + GUARD, dtype=F32, device=c.dev)

    def load(self, key):
        xs = [torch.cat([x[:1], torch.zeros(3)]) for x in inputs((key, "loss"), 4, self.c.world)]
        self.b.fill_(SENT)
        self.b[:4].copy_(xs[self.c.rank])
        self.exp = torch.cat([emu_bucket(xs, False), torch.full((GUARD,), SENT)])

    def issue(self):
        self.c.ar.all_reduce_(self.b[:4])

    def result(self):
        return self.b.cpu()


class _Gather:
    name = "all_gather"

    def __init__(self, c, n):
        self.c, self.n = c, n
        self.x = torch.zeros(n, dtype=BF16, device=c.dev)
        self.b = torch.zeros(n * c.world + GUARD, dtype=BF16, device=c.dev)

    def load(self, key):
        xs = [x.to(BF16) for x in inputs((key, "gather"), self.n, self.c.world)]
        self.b.fill_(SENT)
        self.x.copy_(xs[self.c.rank])
        self.exp = torch.cat(xs + [torch.full((GUARD,), SENT, dtype=BF16)]).view(torch.int16)

    def issue(self):
        self.c.ar.all_gather(self.x, self.b[:self.n * self.c.world])

    def result(self):
        return self.b.cpu().view(torch.int16)


class _EndStep:
    name = "end_step"
    exp = None

    def __init__(self, c):
        self.c = c

    def load(self, key):
        pass

    def issue(self):
        self.c.ar.end_step()

    def result(self):
        return None


class _Ctx:
    def __init__(self, ar, d, path):
        self.ar, self.rank, self.world, self.dev, self.path = ar, d.rank, d.world, d.device, path
        self.reports = []

    def record(self, case, ok, ndiff=0, first=-1, note=""):
        self.reports.append({"case": case, "ok": bool(ok), "ndiff": int(ndiff), "first": int(first), "note": note})
        if not ok:
            self.flush()
            raise AssertionError(f"rank {self.rank}/{self.world} {case}: {ndiff} differ, first at {first} {note}")

    def flush(self):
        with open(self.path, "w") as f:
            json.dump(self.reports, f)

    def verify(self, name, ops):
        torch.cuda.synchronize()
        for i, op in enumerate(ops):
            got = op.result()
            if got is None:
                continue
            assert got.shape == op.exp.shape and got.dtype == op.exp.dtype
            ne = (got != op.exp).reshape(-1)
            nd = int(ne.sum())
            self.record(f"{name}/{i}:{op.name}", nd == 0, nd, int(ne.nonzero()[0]) if nd else -1)
        self.ar.check()  # no barrier timed out, host and device agree on the buffer half
        self.record(f"{name}/check", True)

    def run(self, name, ops, key="eager"):
        for i, op in enumerate(ops):
            op.load((name, i, key))
        for op in ops:
            op.issue()   # no host sync in between
        self.verify(name, ops)


def _sequence(c):
    """7 calls (odd) + end_step: loss sum, bucket, bucket, gather, 3 buckets -- the engine's order, both payloads,
    a capped grid in between; every buffer half is reused three times within one step."""
    W = c.world
    return [_Loss(c), _Bucket(c, 8 * W + 4, True, None), _Bucket(c, 4 * 1031, False, None), _Gather(c, 8 * 131),
            _Bucket(c, 40004, True, 1), _Bucket(c, 8, False, None), _Bucket(c, 8 * 1031, True, 2), _EndStep(c)]


def _validation(c):
    from distributed_training_compare_jax_amd.ops import _native as N

    ar = c.ar
    L, st = N.lib(), N.stream_ptr(c.dev)
    x = torch.zeros(64, device=c.dev)
    call = lambda p, n, bf, mb: L.dtc_dp_allreduce(p, n, bf, ar._bases_ptr, c.rank, c.world, ar.half,  # noqa: E731
                                                   ar.epoch.data_ptr(), ar.err.data_ptr(), mb, st)
    calls, epoch = ar.calls, int(ar.epoch.item())
    bad = {"n%4": call(x.data_ptr(), 6, 0, 64), "n<=0": call(x.data_ptr(), 0, 0, 64),
           "fp32 oversize": call(x.data_ptr(), ar.half // 4 + 4, 0, 64),
           "bf16 oversize": call(x.data_ptr(), ar.half // 2 + 8, 1, 64),
           "misaligned": call(x.data_ptr() + 4, 8, 0, 64), "blocks<1": call(x.data_ptr(), 8, 0, 0),
           "blocks>1024": call(x.data_ptr(), 8, 0, 1025), "null": call(0, 8, 0, 64)}
    torch.cuda.synchronize()
    for k, rc in bad.items():
        c.record(f"validation/{k}", rc == 4001, note=str(rc))
    c.record("validation/nothing_ran", ar.calls == calls and int(ar.epoch.item()) == epoch)


def _worker(out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.parallel.p2p import DP_P2P_BLOCKS, P2PGradReduce

    d = init_distributed("cuda")
    W = d.world
    torch.set_num_threads(max(1, 8 // W))
    # sized like the engine does: the largest bucket's payload (fp32 here), the gather below fits
    ar = P2PGradReduce(dist.group.WORLD, d.rank, W, d.device, [(0, N_BIG), (N_BIG, N_BIG + 40004)], "fp32",
                       gather_bytes=8 * 131 * 2 * W, use_stream=False)
    assert ar.half == (N_BIG * 4 + 4095) // 4096 * 4096 and ar.max_blocks == DP_P2P_BLOCKS
    c = _Ctx(ar, d, os.path.join(out_dir, f"rank{d.rank}.json"))
    for n, mb in sizes(W):
        for bf in (False, True):
            # two calls on different inputs: both buffer halves at every size
            c.run(f"size{n}_{'bf16' if bf else 'f32'}", [_Bucket(c, n, bf, mb), _Bucket(c, n, bf, mb)])
    c.run("production_cap", [_Bucket(c, N_BIG, False, None), _Bucket(c, N_BIG, True, None)])
    assert ar.calls % 2 == 0
    ops = _sequence(c)
    c.run("sequence", ops)
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
        c.verify(f"sequence_graph/replay{r}", ops)
    _validation(c)
    c.flush()
    ar.close()
    destroy()


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("world", WORLDS)
def test_dp_bucket_allreduce_bitwise(cuda, world):
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
    for rep in reps:
        assert [e["case"] for e in rep] == names
    # every size in both payloads twice, the production cap, the sequence eagerly and in 3 replays, the refusals
    assert sum(n.startswith("size") and ":bucket" in n for n in names) == 4 * len(sizes(world))
    assert sum(n.startswith("production_cap/") and ":bucket" in n for n in names) == 2
    for what in ["sequence"] + [f"sequence_graph/replay{r}" for r in range(3)]:
        got = [n for n in names if n.startswith(what + "/")]
        assert sum(":bucket" in n for n in got) == 5 and any(n.endswith(":loss_sum") for n in got)
        assert any(n.endswith(":all_gather") for n in got) and any(n.endswith("/check") for n in got)
    assert sum(n.startswith("validation/") for n in names) == 9
