"""The in-graph xGMI collectives of ``csrc/p2p.hip`` bit for bit, at 2, 3, 5 and 8 ranks (docs/NUMERICS.md).

The kernels only add and convert (no multiply, no fast-math), and the file header fixes the order: every rank
forms the same sum in rank order starting from rank 0; the bf16 two-shot path rounds the reduced slice once to
bf16; the residual and the bias are added after the sum.  A loop of ``s = s + x[p]`` in fp32 torch on the CPU
therefore predicts every output bit.  The emulations below are written from those formulas and from no kernel
output; every worker regenerates every rank's input from seeded generators, computes what it expects itself and
compares on the spot (``!=`` on the values: +0 and -0 compare equal, the inputs hold no NaN; the all-gather is
compared on integer views, it copies arbitrary 16-byte pieces).

One spawned test per world, W processes on one GPU over gloo.  Inputs are ``randn * 10^U(-2, 2)``, different for
every (case, call, replay) and rank, so a stale buffer half, a dropped rank or a wrong order gives wrong bits.
Before call k rank ``k mod W`` sleeps 5 ms on the host, so the ranks do not run in lock step; each case issues
its calls without a host sync in between.  No case provokes a barrier timeout.

The ``test_selfcheck_*`` tests need no GPU.
"""

import functools
import hashlib
import json
import os
import tempfile
import time
import zlib

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

gpu = pytest.mark.gpu
slow = pytest.mark.slow

WORLDS = (2, 3, 5, 8)
MAX_BYTES = 8 * 1024 * 1024 + 12288   # a multiple of 4096: the buffer half is exactly this many bytes
HALF = MAX_BYTES
GUARD = 64                            # sentinel elements behind every output
SENT = 12345.0
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ inputs

def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


STRIDE = 7919


@functools.lru_cache(maxsize=4)
def _scale(n):
    """10^U(-2, 2), fp32 [2 n], the size's n draws twice over: a window [q, q + n) is the vector rotated by q.
    Drawn once per size (the pow is the generator's costly half)."""
    return torch.pow(10.0, torch.rand(n, generator=_gen("scale", n)) * 4 - 2).repeat(2)


def _window(z, rank, n):
    q = STRIDE * (rank + 1) % n
    return z * _scale(n)[q:q + n]


def _inp(key, rank, n, tag="x"):
    """randn * 10^U(-2, 2), fp32 [n].  The normal factor is a function of (key, rank, tag) alone; the scale is the
    size's vector rotated by a rank-dependent offset, so the ranks' magnitudes at one element are unrelated."""
    return _window(torch.randn(n, generator=_gen(key, rank, tag)), rank, n)


def _inp_all(key, n, world):
    """Every rank's input of one call: rank p takes the normal draws [p STRIDE, p STRIDE + n) of ONE stream seeded
    by the key (one generator call per collective call instead of W) times its own rotation of the scale."""
    z = torch.randn(n + STRIDE * world, generator=_gen(key, "all"))
    return [_window(z[p * STRIDE:p * STRIDE + n], p, n) for p in range(world)]


@functools.lru_cache(maxsize=1)
def _inputs(key, n, world):
    """Every rank's fp32 input of one call (kept for the call that repeats it in the other mode)."""
    return tuple(_inp_all(key, n, world))


def _bits(key, rank, n):
    g = _gen(key, rank, "bits")
    return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)


# ------------------------------------------------------------------------------------------------ emulations
# (csrc/p2p.hip: rank_sum_f32 in p2p_reduce_scatter_kernel / p2p_oneshot_kernel; rank_sum_bf16 + finish8;
# p2p_rs_kernel; p2p_ag_kernel)

def emu_sum_f32(xs):
    """fp32 all-reduce, either mode: s = x[0]; s = s + x[p] in rank order."""
    s = xs[0].clone()
    for x in xs[1:]:
        s = s + x
    return s


def emu_acc(xs):
    """a = 0; a += float(x[p]) in rank order (the bf16 paths and the reduce-scatter)."""
    a = torch.zeros(xs[0].numel(), dtype=F32)
    for x in xs:
        a = a + x.reshape(-1).float()
    return a


def emu_finish(a, resid=None, bias=None, ncols=0):
    """+ resid, then + bias[column]; the column of element e is e % ncols (finish8: (8 i) % ncols + lane)."""
    if resid is not None:
        a = a + resid.reshape(-1)
    if bias is not None:
        a = a + bias[torch.arange(a.numel()) % ncols]
    return a


def emu_ar_bf16(xs, resid=None, bias=None, ncols=0, two_shot=False):
    a = emu_acc(xs)
    if two_shot:  # the reduced slice crosses the second barrier as bf16: one round-to-nearest-even
        a = a.to(BF16).float()
    return emu_finish(a, resid, bias, ncols)


def emu_rs(xs, rank, world, resid=None, bias=None, ncols=0):
    """This rank's n_loc elements; resid holds this rank's rows, the bias column is the local (8 i) % ncols."""
    n_loc = xs[0].numel() // world
    sl = slice(rank * n_loc, (rank + 1) * n_loc)
    return emu_finish(emu_acc([x.reshape(-1)[sl] for x in xs]), resid, bias, ncols)


def emu_ag(xs):
    return torch.cat([x.reshape(-1) for x in xs])


def oneshot_auto(nbytes, world):
    """The documented mode-0 rule: one-shot at W = 2, up to 1 MiB of payload at W <= 4, 512 KiB above."""
    return world <= 2 or nbytes <= (1 << 20 if world <= 4 else 1 << 19)


def compare(got, exp):
    """(number of differing elements, first differing index or -1)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    ne = (got != exp).reshape(-1)
    nd = int(ne.sum())
    return nd, (int(ne.nonzero()[0]) if nd else -1)


def _ar_f32_sizes(W):
    return list(dict.fromkeys([4, 4 * (W - 1), 4 * (W + 1), 4 * (1000 * W + 1), HALF // 4]))


def _ar_bf16_sizes(W):
    return list(dict.fromkeys([8, 8 * (W - 1), 8 * (W + 1), 24 * 131]))


def _ag_sizes(W):
    return [16, 16 * 1031, HALF // (16 * W) * 16]  # the last: W * loc_bytes == half where W divides it


# ------------------------------------------------------------------------------------------------ worker side

class _Ctx:
    def __init__(self, ar, rank, world, dev, path):
        self.ar, self.rank, self.world, self.dev, self.path = ar, rank, world, dev, path
        self.k = 0
        self.reports = []
        self._eye = {}
        self.t0 = self.t_last = time.time()
        self.times = []

    def mark(self, phase):
        now = time.time()
        self.times.append(f"{phase} {now - self.t_last:.2f}")
        self.t_last = now

    def skew(self):
        if self.k % self.world == self.rank:
            time.sleep(0.005)
        self.k += 1

    def buf(self, n, dtype=F32):
        return torch.full((n + GUARD,), _sent(dtype), dtype=dtype, device=self.dev)

    def eye(self, n):
        if n not in self._eye:
            self._eye[n] = torch.eye(n, dtype=BF16, device=self.dev)
        return self._eye[n]

    def flush(self):
        with open(self.path, "w") as f:
            json.dump(self.reports, f)

    def record(self, case, ok, ndiff=0, first=-1, sha=None, note=""):
        self.reports.append({"case": case, "ok": bool(ok), "ndiff": ndiff, "first": first, "sha": sha, "note": note})
        if not ok:
            self.flush()
            raise AssertionError(f"rank {self.rank}/{self.world} {case}: {ndiff} elements differ, first at {first} {note}")

    def verify(self, name, ops, same=()):
        """One host sync for the whole case, every op against its expectation, then the error word."""
        torch.cuda.synchronize()
        got = [op.result() for op in ops]
        bad = None
        for i, (op, g) in enumerate(zip(ops, got)):
            if g is None:
                continue
            nd, first = compare(g, op.exp)
            sha = hashlib.sha256(g.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() if op.allrank else None
            self.reports.append({"case": f"{name}/{i}:{op.name}", "ok": nd == 0, "ndiff": nd, "first": first, "sha": sha,
                                 "note": ""})
            if nd and bad is None:
                bad = self.reports[-1]
        for i, j in same:
            nd, first = compare(got[i], got[j])
            self.reports.append({"case": f"{name}/{i}=={j}", "ok": nd == 0, "ndiff": nd,
                                 "first": first, "sha": None, "note": ""})
            bad = bad or (self.reports[-1] if nd else None)
        self.flush()
        if bad is not None:
            raise AssertionError(f"rank {self.rank}/{self.world}: {bad}")
        self.ar.check()

    def run(self, name, ops, keys=None, same=()):
        """Eager: load every input, issue the whole sequence without a host sync, then compare."""
        for i, op in enumerate(ops):
            op.load((name, keys[i] if keys else i, "eager"))
        for op in ops:
            self.skew()
            op.issue()
        self.verify(name, ops, same)

    def capture(self, ops):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin(capture_error_mode="thread_local")
            for op in ops:
                op.issue()
            g.capture_end()
        torch.cuda.current_stream().wait_stream(s)
        return g

    def run_graph(self, name, ops, replays=3):
        g = self.capture(ops)
        for r in range(replays):
            for i, op in enumerate(ops):
                op.load((name, i, "replay", r))
            self.skew()
            g.replay()
            self.verify(f"{name}/replay{r}", ops)


class _Op:
    allrank = True   # the same output on every rank (hashed and compared across ranks)
    exp = None

    def load(self, key):
        pass

    def result(self):
        return None


def _sent(dtype):
    return SENT if dtype.is_floating_point else int(SENT)


def _guarded(exp):
    return torch.cat([exp, torch.full((GUARD,), _sent(exp.dtype), dtype=exp.dtype)])


class _ArF32(_Op):
    def __init__(self, c, n, mode):
        self.c, self.n, self.mode, self.name = c, n, mode, f"ar_f32[n={n},mode={mode}]"
        self.b = c.buf(n)
        self.t = self.b[:n]

    def load(self, key):
        xs = _inputs(key, self.n, self.c.world)
        self.t.copy_(xs[self.c.rank])
        self.exp = _guarded(emu_sum_f32(xs))

    def issue(self):
        self.c.ar.all_reduce_(self.t, self.mode)

    def result(self):
        return self.b.cpu()


class _ArBf16(_Op):
    """all_reduce_bf16 of n elements; ``ncols`` > 0 adds a bias (the output is then viewed as [-1, ncols] and may
    end in a partial row the kernel must not write); ``staged``: (rows, cols), the payload is written by a GEMM
    with the identity into ``staged_out`` and the call runs with ``x=None``.  ``two_shot`` is what the emulation
    assumes: the test states it, the kernel is never asked."""

    def __init__(self, c, n, mode, resid, ncols, two_shot, staged=None):
        self.c, self.mode, self.two_shot, self.staged = c, mode, two_shot, staged
        if staged:
            n = staged[0] * staged[1]
            ncols = staged[1] if ncols else 0
        self.n, self.ncols = n, ncols
        self.name = f"ar_bf16[n={n},mode={mode},resid={int(resid)},ncols={ncols},staged={int(bool(staged))}]"
        padded = -(-n // ncols) * ncols if ncols else n
        self.b = c.buf(padded)
        self.padded = padded
        self.out = self.b[:n].view(staged) if staged else (self.b[:padded].view(-1, ncols) if ncols else self.b[:n])
        self.x = torch.empty(staged if staged else (n,), dtype=BF16, device=c.dev)
        self.rs = torch.empty(n, device=c.dev) if resid else None
        self.bs = torch.empty(ncols, device=c.dev) if ncols else None
        if staged:
            c.eye(staged[1])

    def load(self, key):
        xs = [x.to(BF16) for x in _inp_all(key, self.n, self.c.world)]
        rs = _inp(key, -1, self.n, "resid") if self.rs is not None else None
        bs = _inp(key, -1, self.ncols, "bias") if self.bs is not None else None
        self.b.fill_(_sent(self.b.dtype))
        self.x.copy_(xs[self.c.rank].view(self.x.shape))
        if rs is not None:
            self.rs.copy_(rs)
        if bs is not None:
            self.bs.copy_(bs)
        exp = emu_ar_bf16(xs, rs, bs, self.ncols, self.two_shot)
        self.exp = _guarded(torch.cat([exp, torch.full((self.padded - self.n,), SENT)]))

    def issue(self):
        ar = self.c.ar
        if self.staged:
            from distributed_training_compare_jax_amd.ops.gemm import linear_into

            linear_into(self.x, self.c.eye(self.staged[1]), ar.staged_out(self.n))
            ar.all_reduce_bf16(None, self.out, self.rs, self.bs, mode=self.mode)
        else:
            ar.all_reduce_bf16(self.x, self.out, self.rs, self.bs, mode=self.mode)

    def result(self):
        return self.b.cpu()


class _Rs(_Op):
    allrank = False

    def __init__(self, c, rows, cols, dtype, resid, bias, staged=False):
        self.c, self.rows, self.cols, self.dtype, self.staged = c, rows, cols, dtype, staged
        self.n, self.n_loc = rows * cols, rows // c.world * cols
        dn = "bf16" if dtype == BF16 else "f32"
        self.name = f"rs_{dn}[{rows}x{cols},resid={int(resid)},bias={int(bias)},staged={int(staged)}]"
        self.b = c.buf(self.n_loc)
        self.out = self.b[:self.n_loc].view(rows // c.world, cols)
        self.x = torch.empty(rows, cols, dtype=BF16 if staged else dtype, device=c.dev)
        self.rs = torch.empty(self.n_loc, device=c.dev) if resid else None
        self.bs = torch.empty(cols, device=c.dev) if bias else None
        if staged:
            c.eye(cols)

    def load(self, key):
        c = self.c
        # a staged fp32 partial is what the GEMM makes of bf16 inputs: bf16 values held in fp32
        xs = [x.to(BF16 if self.staged else self.dtype).to(self.dtype) for x in _inp_all(key, self.n, c.world)]
        rs = _inp(key, c.rank, self.n_loc, "resid") if self.rs is not None else None  # this rank's rows
        bs = _inp(key, -1, self.cols, "bias") if self.bs is not None else None
        self.b.fill_(_sent(self.b.dtype))
        self.x.copy_(xs[c.rank].view(self.rows, self.cols))
        if rs is not None:
            self.rs.copy_(rs)
        if bs is not None:
            self.bs.copy_(bs)
        self.exp = _guarded(emu_rs(xs, c.rank, c.world, rs, bs, self.cols))

    def issue(self):
        ar = self.c.ar
        if self.staged:
            from distributed_training_compare_jax_amd.ops.gemm import linear_into

            linear_into(self.x, self.c.eye(self.cols), ar.staged_out(self.n, self.dtype))
            ar.reduce_scatter(None, self.rows, self.cols, self.dtype, self.out, self.rs, self.bs)
        else:
            ar.reduce_scatter(self.x, self.rows, self.cols, self.dtype, self.out, self.rs, self.bs)

    def result(self):
        return self.b.cpu()


class _Ag(_Op):
    def __init__(self, c, loc_bytes, kind):
        self.c, self.kind = c, kind
        self.dtype, self.view = (torch.int32, torch.int32) if kind == "i32" else (BF16, torch.int16)
        self.n = loc_bytes // (4 if kind == "i32" else 2)
        self.name = f"ag_{kind}[loc_bytes={loc_bytes}]"
        self.x = torch.empty(self.n, dtype=self.dtype, device=c.dev)
        self.b = c.buf(self.n * c.world, self.dtype)

    def load(self, key):
        c = self.c
        if self.kind == "i32":  # arbitrary bit patterns, NaN payloads included
            xs = [_bits(key, p, self.n) for p in range(c.world)]
        else:
            xs = [x.to(BF16) for x in _inp_all(key, self.n, c.world)]
        self.b.fill_(_sent(self.b.dtype))
        self.x.copy_(xs[c.rank])
        self.exp = _guarded(emu_ag(xs)).view(self.view)

    def issue(self):
        self.c.ar.all_gather(self.x, self.b[:self.n * self.c.world])

    def result(self):
        return self.b.cpu().view(self.view)


class _EndStep(_Op):
    name = "end_step"

    def __init__(self, c):
        self.c = c

    def issue(self):
        self.c.ar.end_step()


def _mixed_ops(c):
    """15 calls and 3 end_step rounds with no sync: two- and one-barrier calls behind each other, staged and
    copied payloads, every buffer half reused nine times.  Each round is 5 calls + 1 padding round: even."""
    W = c.world
    ops = []
    for r in range(3):
        ops += [_ArF32(c, [4 * (W + 1), 4 * (1000 * W + 1), 4096 * 3][r], 1),
                _ArF32(c, [4 * (1000 * W + 1), 4, 4 * (W - 1)][r], 2),
                _ArBf16(c, 0, [2, 1, 1][r], True, 64, [False, True, True][r], staged=(3 * 256, 64)),
                _Rs(c, W * 128, 64, [BF16, F32, BF16][r], True, True, staged=(r == 1)),
                _Ag(c, [16 * 1031, 16, 16 * 1031][r], ["i32", "bf16", "i32"][r]),
                _EndStep(c)]
    return ops


def _raises(fn, match):
    try:
        fn()
    except RuntimeError as e:
        return match in str(e), str(e)
    return False, "no RuntimeError"


def _phase_validation(c):
    """Refused arguments raise on every rank, launch nothing and leave the call count and the epoch alone."""
    from distributed_training_compare_jax_amd.ops import _native as N

    ar, dev, W = c.ar, c.dev, c.world
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    h = lambda *s: torch.empty(*s, dtype=BF16, device=dev)  # noqa: E731

    def rs_partial_rows():  # n_loc % ncols != 0 cannot be spelled through reduce_scatter(rows, cols): the C entry
        out, x, b = f(8), h(8 * W), f(16)
        N.check(N.lib().dtc_p2p_reduce_scatter(x.data_ptr(), 1, out.data_ptr(), 8, ar._bases_ptr, c.rank, W, ar.half,
                                               ar.epoch.data_ptr(), ar.err.data_ptr(), 0, b.data_ptr(), 16,
                                               N.stream_ptr(dev)), "dtc_p2p_reduce_scatter")

    nl = 262656  # at W = 2 the [2 * 262,656, 8] bf16 partial is 8,404,992 bytes: 4096 more than the half
    bad = {
        "n%4": lambda: ar.all_reduce_(f(6)),
        "n*4>half": lambda: ar.all_reduce_(f(HALF // 4 + 4)),
        "bf16 n%8": lambda: ar.all_reduce_bf16(h(12), f(12)),
        "bf16 n*2>half": lambda: ar.all_reduce_bf16(h(HALF // 2 + 8), f(HALF // 2 + 8)),
        "bias ncols%8": lambda: ar.all_reduce_bf16(h(24), f(2, 12), None, f(12)),
        "rs n_loc%ncols": rs_partial_rows,
        "rs oversize": lambda: ar.reduce_scatter(h(nl * W, 8), nl * W, 8, BF16, f(nl, 8)),
        "ag bytes%16": lambda: ar.all_gather(f(6), f(6 * W)),
        "rs rows%W": lambda: ar.reduce_scatter(h(W + 1, 8), W + 1, 8, BF16, f(1, 8)),
    }
    for name, fn in bad.items():
        calls, epoch = ar.calls, int(ar.epoch.item())
        ok, msg = _raises(fn, "do not divide" if name == "rs rows%W" else "failed with HIP error code 4001")
        c.record(f"validation/{name}", ok and ar.calls == calls and int(ar.epoch.item()) == epoch, note=msg)
    c.run("validation/next_valid", [_ArF32(c, 4 * (W + 1), 1), _ArBf16(c, 8 * (W + 1), 2, True, 8, False)])


def _phase_check(c):
    """The buffer-half invariant of check(): host bookkeeping only, every kernel issued is well formed."""
    from distributed_training_compare_jax_amd.ops import _native as N

    ar, W = c.ar, c.world
    ar.end_step()
    ar.check()
    assert ar.calls % 2 == 0
    op = _ArF32(c, 4 * (W + 1), 1)
    g = c.capture([op])          # one call, no end_step: the host counts it once, nothing has run
    for r in range(2):           # two replays advance the device epoch by 4: host half 1, device half 0
        op.load(("check", r))
        c.skew()
        g.replay()
    torch.cuda.synchronize()
    nd, first = compare(op.result(), op.exp)   # the call itself stages by the device epoch: still right
    c.record("check/odd_graph_second_replay", nd == 0, nd, first)
    ok, msg = _raises(ar.check, "buffer-half mismatch")
    c.record("check/mismatch_raises", ok, note=msg)
    ar.end_step()                # counted on both sides (host + 1, epoch + 2): the two halves still differ
    ok, msg = _raises(ar.check, "buffer-half mismatch")
    c.record("check/end_step_alone_keeps_mismatch", ok, note=msg)
    c.skew()                     # a barrier round the host does not count brings the device half back
    N.check(N.lib().dtc_p2p_barrier_round(ar._bases_ptr, c.rank, W, ar.epoch.data_ptr(), ar.err.data_ptr(),
                                          N.stream_ptr(c.dev)), "dtc_p2p_barrier_round")
    ok = True
    try:
        ar.check()
    except RuntimeError as e:
        ok, msg = False, str(e)
    c.record("check/repaired", ok and ar.calls % 2 == 0, note="" if ok else msg)
    # staged_out is computed from the host half: right bits again only if host and device agree
    c.run("check/staged_after_repair", [_ArBf16(c, 0, 2, True, 64, False, staged=(3 * 256, 64)),
                                        _ArBf16(c, 0, 1, True, 64, True, staged=(3 * 256, 64))])


def _phase_tpcomm(c):
    """parallel/tp.py routing: the stub program raises on any process-group collective, so a pass proves that
    every call took the in-graph kernels."""
    from distributed_training_compare_jax_amd.parallel.tp import TPComm

    class _NoComm:
        def comm(self, *a, **k):
            raise AssertionError("TPComm fell back to a process-group collective")

    ar, W, rank, dev = c.ar, c.world, c.rank, c.dev
    tp = TPComm(None, W, rank, _NoComm(), p2p=ar)

    def rec(name, got, exp, allrank=True):
        got = got.cpu()
        nd, first = compare(got.reshape(-1), exp.reshape(-1))
        sha = hashlib.sha256(got.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() if allrank else None
        c.record(f"tpcomm/{name}", nd == 0, nd, first, sha)

    for k in (1, 2, 3, 4):       # fewer than 4: the zero-padded 4-float route
        xs = [_inp(("tp_ar", k), p, k) for p in range(W)]
        t = xs[rank].to(dev)
        c.skew()
        tp.all_reduce_(t)
        rec(f"all_reduce_[{k}]", t, emu_sum_f32(xs))
    for shape in ((2,), (197, 2), (1,)):   # CE row statistics, a label-logit vector
        n = 1
        for s in shape:
            n *= s
        xs = [_inp(("tp_stack", shape), p, n).view(shape) for p in range(W)]
        xs[W - 1].view(-1)[0] = -0.0       # comes back as +0.0: equal numerically
        c.skew()
        got = tp.all_gather_stack(xs[rank].to(dev))
        assert tuple(got.shape) == (W,) + shape
        rec(f"all_gather_stack{list(shape)}", got, torch.stack(xs))
    xs = [_inp("tp_reduce_to", p, 6 * 24).to(BF16).view(6, 24) for p in range(W)]
    rs, bs = _inp("tp_reduce_to", -1, 6 * 24, "resid").view(6, 24), _inp("tp_reduce_to", -1, 24, "bias")
    c.skew()
    got = tp.reduce_to(xs[rank].to(dev), rs.to(dev), bs.to(dev))
    rec("reduce_to", got, emu_ar_bf16(xs, rs, bs, 24, two_shot=False))  # 288 bytes: one-shot at every W
    xs = [_inp("tp_rs_rows", p, 3 * W * 24).to(BF16).view(3 * W, 24) for p in range(W)]
    rs, bs = _inp("tp_rs_rows", rank, 3 * 24, "resid").view(3, 24), _inp("tp_rs_rows", -1, 24, "bias")
    c.skew()
    got = tp.reduce_scatter_rows(xs[rank].to(dev), rs.to(dev), bs.to(dev))
    rec("reduce_scatter_rows", got, emu_rs(xs, rank, W, rs, bs, 24), allrank=False)
    xs = [_inp("tp_ag_rows", p, 3 * 8).view(3, 8) for p in range(W)]
    c.skew()
    got = tp.all_gather_rows(xs[rank].to(dev))
    assert tuple(got.shape) == (3 * W, 8)
    rec("all_gather_rows", got, emu_ag(xs))
    # the staging hooks return None exactly where their docstrings say
    b8, b12 = torch.zeros(8, device=dev), torch.zeros(12, device=dev)
    own = ar._own + ar._flag_bytes + (ar.calls & 1) * ar.half
    none = {
        "partial_out bias cols%8": tp.partial_out(8, 12, b12),
        "partial_out oversize": tp.partial_out(HALF // 16 + 8, 8),
        "partial_out_rows rows%W": tp.partial_out_rows(W + 1, 8, BF16),
        "partial_out_rows bias cols%8": tp.partial_out_rows(2 * W, 12, BF16, b12),
        "partial_out_rows oversize": tp.partial_out_rows(W * (HALF // (16 * W) + 1), 8, BF16),
        "staged_out numel%8": ar.staged_out(12),
        "staged_out oversize": ar.staged_out(HALF // 2 + 8),
        "staged_out fp32 oversize": ar.staged_out(HALF // 4 + 8, F32),
        "staged_out dtype": ar.staged_out(8, torch.float16),
    }
    some = {
        "partial_out": tp.partial_out(8, 12),
        "partial_out bias": tp.partial_out(8, 8, b8),
        "partial_out exact": tp.partial_out(HALF // 16, 8),
        "partial_out_rows": tp.partial_out_rows(2 * W, 12, BF16),
        "partial_out_rows fp32": tp.partial_out_rows(2 * W, 8, F32, b8),
        "staged_out exact": ar.staged_out(HALF // 2),
    }
    for k, v in none.items():
        c.record(f"tpcomm/none/{k}", v is None)
    for k, v in some.items():
        c.record(f"tpcomm/some/{k}", v is not None and v.ptr == own)
    ar.end_step()
    torch.cuda.synchronize()
    ar.check()
    c.flush()


def _worker(out_dir, t_parent):
    t_start = time.time()
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.parallel.p2p import P2PAllReduce

    d = init_distributed("cuda")
    W = d.world
    torch.set_num_threads(max(1, 8 // W))  # W processes share the host with their runtime threads
    ar = P2PAllReduce(dist.group.WORLD, d.rank, W, d.device, MAX_BYTES)
    assert ar.half == HALF
    c = _Ctx(ar, d.rank, W, d.device, os.path.join(out_dir, f"rank{d.rank}.json"))
    c.t_last = t_start
    c.mark("init")

    # fp32 all-reduce: both modes on different inputs, then mode 2 again on mode 1's input (same bits)
    for n in _ar_f32_sizes(W):
        c.run(f"ar_f32/{n}", [_ArF32(c, n, 1), _ArF32(c, n, 2), _ArF32(c, n, 2)], keys=[0, 1, 0], same=[(0, 2)])
    c.mark("ar_f32")
    # bf16 all-reduce: plain, resid, bias at ncols 8, both at ncols 24
    for resid, ncols in ((False, 0), (True, 0), (False, 8), (True, 24)):
        c.run(f"ar_bf16/resid{int(resid)}_ncols{ncols}",
              [_ArBf16(c, n, m, resid, ncols, m == 1) for n in _ar_bf16_sizes(W) for m in (1, 2)])
    # mode 0 at the one-shot threshold and 16 bytes above it
    thr = (1 << 20) if W <= 4 else (1 << 19)
    c.run("ar_bf16/auto_threshold", [_ArBf16(c, thr // 2, 0, True, 0, not oneshot_auto(thr, W)),
                                     _ArBf16(c, thr // 2 + 8, 0, True, 0, not oneshot_auto(thr + 16, W))])
    c.mark("ar_bf16")
    # payloads written in place by a GEMM
    c.run("staged", [_ArBf16(c, 0, 1, True, 64, True, staged=(3 * 256, 64)),
                     _ArBf16(c, 0, 2, True, 64, False, staged=(3 * 256, 64)),
                     _Rs(c, W * 128, 64, BF16, True, True, staged=True),
                     _Rs(c, W * 128, 64, F32, True, True, staged=True)])
    c.mark("staged")
    # reduce-scatter
    for dt, dn in ((BF16, "bf16"), (F32, "f32")):
        c.run(f"rs_{dn}", [_Rs(c, rows, cols, dt, resid, bias)
                           for rows, cols in ((W, 8), (3 * W, 24), (W * 128, 64))
                           for resid, bias in ((False, False), (True, False), (False, True), (True, True))])
    if W == 2:
        # n_loc = 8 * 262,528: the [2 * 262,528, 8] bf16 partial fills the half exactly, and the 262,144
        # threads of p2p_rs_kernel's capped grid go round a second time (384 of them)
        c.run("rs_bf16/second_pass", [_Rs(c, HALF // 16, 8, BF16, True, True)])
    c.mark("rs")
    # all-gather
    c.run("ag", [_Ag(c, nb, kind) for nb in _ag_sizes(W) for kind in ("i32", "bf16")])
    # the mixed sequence, eager and then as one hipGraph with end_step inside the capture
    c.mark("ag")
    ar.end_step()  # a step starts on an even call count (the engine ends every step with end_step)
    ops = _mixed_ops(c)
    c.run("mixed", ops)
    c.run_graph("mixed_graph", ops)
    del ops
    c.mark("mixed")
    _phase_validation(c)
    _phase_check(c)
    _phase_tpcomm(c)
    c.mark("validation+check+tpcomm")
    ar.close()
    destroy()
    c.mark("close")
    if d.rank == 0:  # where the time goes (pytest -s shows it)
        print(f"P2P-TIMES W={W}: worker entered {t_start - t_parent:.2f} s after the parent's spawn, "
              + ", ".join(c.times) + f", left after {time.time() - t_parent:.2f}")


@gpu
@slow
@pytest.mark.parametrize("world", WORLDS)
def test_p2p_collectives_bitwise(cuda, world):
    """Every case bit for bit on every rank, check() clean after every case, the same all-reduce output (SHA-256)
    on every rank.  Measured on an MI355X: see docs/NUMERICS.md, "Collectives"."""
    err = None
    with tempfile.TemporaryDirectory() as td:
        t0 = time.time()
        try:
            spawn(_worker, world, args=(td, t0))
        except Exception as e:  # a worker raised at its first mismatch: show what the reports hold
            err = e
        reps = []
        for r in range(world):
            p = os.path.join(td, f"rank{r}.json")
            reps.append(json.load(open(p)) if os.path.exists(p) else None)
    print(f"P2P-TIMES W={world}: spawn returned after {time.time() - t0:.2f}")
    bad = [(r, e) for r, rep in enumerate(reps) if rep for e in rep if not e["ok"]]
    assert err is None and not bad, f"world {world}: {bad[:8]} {err}"
    assert all(rep for rep in reps)
    names = [e["case"] for e in reps[0]]
    assert len(names) == len(set(names)) and len(names) > 150
    for r, rep in enumerate(reps):
        assert [e["case"] for e in rep] == names, r
        for e0, e in zip(reps[0], rep):
            assert e["sha"] == e0["sha"], (r, e["case"])
    assert sum(e["sha"] is not None for e in reps[0]) > 80


# ------------------------------------------------------------------------------------------------ CPU self-checks

def _xs(W, n, key="self"):
    return _inp_all(key, n, W)


@pytest.mark.parametrize("W", (3, 5, 8))
def test_selfcheck_emulation_is_the_float64_sum_to_fp32_accuracy(W):
    n = 24 * 131 * 8
    xs = _xs(W, n)
    ref = sum(x.double() for x in xs)
    mag = sum(x.double().abs() for x in xs)
    err = (emu_sum_f32(xs).double() - ref).abs()
    assert bool((err <= W * 2.0 ** -24 * mag).all()), float((err / mag).max() / 2.0 ** -24)
    err = (emu_acc(xs).double() - ref).abs()
    assert bool((err <= W * 2.0 ** -24 * mag).all())
    xb = [x.to(BF16) for x in xs]
    ref = sum(x.double() for x in xb)
    mag = sum(x.double().abs() for x in xb)
    # two-shot: one round-to-nearest-even to bf16 (8 significant bits) of the fp32 sum a, i.e. at most half a
    # bf16 ulp of a = 2^-8 * 2^floor(log2 |a|) <= 2^-8 |a|.  (2^-9 |sum| is not a bound of that rounding:
    # 74.25 = -6.375 - 10.375 + 91 lies between the bf16 neighbours 74 and 74.5 and moves by 0.25 = 2^-8.2 of
    # itself; 27 % of these elements exceed 2^-9 |sum|.)
    a = emu_acc(xb)
    half_ulp = torch.ldexp(torch.ones(a.numel(), dtype=torch.float64), torch.frexp(a)[1] - 9)
    err = (emu_ar_bf16(xb, two_shot=True).double() - ref).abs()
    over = float((err > 2.0 ** -9 * ref.abs() + W * 2.0 ** -24 * mag).double().mean())
    print(f"TWO-SHOT W={W}: worst err / half ulp {float((err / half_ulp).max()):.4f}, above 2^-9 |sum|: {over:.3f}")
    assert bool((err <= half_ulp + W * 2.0 ** -24 * mag).all())
    assert bool((half_ulp <= 2.0 ** -8 * a.abs().double())[a != 0].all())


@pytest.mark.parametrize("W", (3, 5, 8))
def test_selfcheck_reverse_order_differs(W):
    """A bitwise pass says something about the order: on these inputs the reverse-order sum has other bits in at
    least 10 % of the elements (measured 25 to 59 %)."""
    xs = _xs(W, 24 * 131 * 8)
    nd, _ = compare(emu_sum_f32(xs[::-1]), emu_sum_f32(xs))
    print(f"REVERSE W={W}: {nd / xs[0].numel():.3f}")
    assert nd >= 0.10 * xs[0].numel()
    xb = [x.to(BF16) for x in xs]
    one, two = emu_ar_bf16(xb), emu_ar_bf16(xb, two_shot=True)
    assert compare(one, two)[0] >= 0.90 * one.numel()  # which path ran is visible in the value


@pytest.mark.parametrize("W", WORLDS)
def test_selfcheck_comparison_rejects_wrong_collectives(W):
    differs = lambda a, b: compare(a, b)[0] > 0  # noqa: E731
    # fp32 all-reduce
    n = 4 * (1000 * W + 1)
    xs = _xs(W, n)
    exp = emu_sum_f32(xs)
    assert compare(exp, emu_sum_f32(_xs(W, n)))[0] == 0
    assert differs(emu_sum_f32(xs[:-1]), exp)                       # the last rank dropped
    if W >= 3:
        assert differs(emu_sum_f32(xs[::-1]), exp)                  # reverse rank order
    floor4 = (n // 4) // W * W * 4                                  # floor instead of ceil chunks:
    tail = exp.clone()                                              # the tail vector elements stay unreduced
    tail[floor4:] = xs[0][floor4:]
    assert floor4 < n and differs(tail, exp)
    assert differs(emu_sum_f32(_xs(W, n, key="two calls earlier")), exp)  # the same half two calls earlier
    # bf16 all-reduce with resid and bias at ncols 24
    n = 24 * 131
    xb = [x.to(BF16) for x in _xs(W, n)]
    rs, bs = _inp("self", -1, n, "resid"), _inp("self", -1, 24, "bias")
    for two in (False, True):
        exp = emu_ar_bf16(xb, rs, bs, 24, two)
        a = emu_ar_bf16(xb, rs, None, 0, two)
        for _ in range(W):
            a = a + bs[torch.arange(n) % 24]
        assert differs(a, exp)                                      # the bias added W times
        # the column taken from the vector index i instead of 8 i: passes at ncols 8 (always column 0 .. 7),
        # which is why the bias cases include ncols 24
        col = (torch.arange(n) // 8 % 24 // 8 * 8 + torch.arange(n) % 8)
        assert differs(emu_ar_bf16(xb, rs, None, 0, two) + bs[col], exp)
    one, two = emu_ar_bf16(xb, rs, bs, 24, False), emu_ar_bf16(xb, rs, bs, 24, True)
    assert differs(one, two)                                        # the two-shot result left unrounded
    assert differs(two.to(BF16).float(), two)                       # rounded again after resid + bias
    # reduce-scatter
    rows, cols = 3 * W, 24
    xp = [x.to(BF16) for x in _xs(W, rows * cols)]
    res = [_inp("self", r, 3 * cols, "resid") for r in range(W)]
    for r in range(W):
        exp = emu_rs(xp, r, W, res[r], bs, cols)
        # whole rows per rank: the global element offset r * n_loc is a multiple of ncols, so "global" and
        # "local" bias columns coincide at every shape the host accepts; the residual rows are what can be confused
        glob = emu_finish(emu_acc([x[r * 3 * cols:(r + 1) * 3 * cols] for x in xp]), res[r])
        glob = glob + bs[(torch.arange(3 * cols) + r * 3 * cols) % cols]
        assert not differs(glob, exp)
        shifted = emu_finish(emu_acc([x[r * 3 * cols:(r + 1) * 3 * cols] for x in xp]), res[r])
        shifted = shifted + bs[(torch.arange(3 * cols) + 8 * r) % cols]   # offset in vector elements, not rows
        if r % 3:
            assert differs(shifted, exp)
        if r:
            assert differs(emu_rs(xp, r, W, res[0], bs, cols), exp)  # rank 0's residual rows on every rank
            assert differs(emu_rs(xp, 0, W, res[r], bs, cols), exp)  # slice 0 instead of slice r
    # all-gather: two slots swapped
    bits = [_bits("self", p, 4 * 1031) for p in range(W)]
    sw = list(bits)
    sw[0], sw[W - 1] = sw[W - 1], sw[0]
    assert differs(emu_ag(sw), emu_ag(bits))
