"""The in-graph pipeline messages (``csrc/p2p.hip`` dtc_pp_send / dtc_pp_recv, ``parallel.p2p.P2PPipe``) bit for bit.

One spawned test per world W: W processes on one GPU over gloo form a chain of stages.  Every case builds a
``P2PPipe`` and runs steps of a real stage program (``parallel.pp.pp_program``, the order ``check_slot_reuse``
proves safe): a post sends its tags, a wait pulls the receives of the posts it names -- what ``run_pipeline`` does.
The messages only copy, so the receiver regenerates the SENDER's payload from a seeded generator keyed on (case,
step, tag, microbatch, sender) and compares integer views on the spot; the payloads are arbitrary bit patterns
(NaNs included) and differ every step, so a stale slot, a wrong offset or a missed wait gives wrong bits.  Guard
sentinels sit behind every destination.  Each case runs eager steps and then one captured step replayed with fresh
payloads written before each replay.  Before step k rank ``k mod W`` sleeps 5 ms on the host.  No case provokes a
spin timeout; ``check()`` is clean after every step.
"""

import json
import os
import tempfile
import time
import zlib

import pytest
import torch

from distributed_training_compare_jax_amd.parallel.dist import spawn

WORLDS = (2, 3, 4, 8)
GUARD = 64
BF16, F32 = torch.bfloat16, torch.float32
ROWS, T, D = 2, 64, 64            # the tiny model at batch 4, 2 microbatches: mb_rows * T * D elements per message
TINY = ROWS * T * D
EAGER_STEPS, REPLAYS = 3, 5

# (name, schedule, microbatches, head split, message shapes): 16 B, 16 * (odd) B and the tiny model's message in
# bf16 and fp32; the head split adds the compute-dtype f message of the last pair and the [rows, 3] fp32 statistics
CASES = [
    ("tiny_bf16_split", "1f1b", 2, True, {"f": (TINY, BF16), "b": (TINY, BF16), "fh": (TINY, BF16),
                                          "s": (ROWS * T * 3, F32)}),
    ("b16", "gpipe", 3, False, {"f": (4, F32), "b": (8, BF16)}),
    ("odd", "1f1b", 2, False, {"f": (4 * 131, F32), "b": (8 * 1031, BF16)}),
    ("tiny_f32", "gpipe", 4, False, {"f": (TINY, F32), "b": (TINY, F32)}),
]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def payload(case, step, tag, i, sender, nbytes):
    """Arbitrary bits, int32 [nbytes / 4]."""
    g = _gen(case, step, tag, i, sender)
    return torch.randint(-2 ** 31, 2 ** 31, (nbytes // 4,), generator=g, dtype=torch.int64).to(torch.int32)


def finite_bf16(case, step, tag, i, sender, n):
    """Finite bf16 values (a message its producer writes through a GEMM with the identity)."""
    return (torch.randn(n, generator=_gen(case, step, tag, i, sender, "finite")) * 8).to(BF16)


def f32_image_bits(bits_i32):
    """The fp32 image of a bf16 message given as int32 words: element 2k is the low half, 2k + 1 the high half."""
    lo = bits_i32 << 16
    hi = bits_i32 & -65536
    return torch.stack([lo, hi], dim=1).reshape(-1)


def test_selfcheck_f32_image_is_float_of_bf16():
    bits = payload("self", 0, "f", 0, 0, 4096)
    assert torch.equal(f32_image_bits(bits), bits.view(BF16).float().view(torch.int32))
    assert not torch.equal(payload("self", 1, "f", 0, 0, 4096), bits)
    assert not torch.equal(payload("self", 0, "f", 0, 1, 4096), bits)


class _Case:
    def __init__(self, name, kind, M, hs, msgs, d, report):
        import torch.distributed as dist

        from distributed_training_compare_jax_amd.parallel.p2p import P2PPipe
        from distributed_training_compare_jax_amd.parallel.pp import pp_program

        self.name, self.M, self.hs, self.rank, self.W, self.dev = name, M, hs, d.rank, d.world, d.device
        self.report = report
        self.pipe = P2PPipe(dist.group.WORLD, d.rank, d.world, d.device, M, hs, msgs)
        self.prog = pp_program(kind, d.world, d.rank, M, head_split=hs)
        self.rcv = {it[1]: it[4] for it in self.prog if it[0] == "post"}
        t = self.pipe.table
        self.src = {k: torch.zeros(e.nbytes // 4, dtype=torch.int32, device=self.dev) for k, e in t["send"].items()}
        self.dst = {k: torch.zeros(e.nbytes // 4 + GUARD, dtype=torch.int32, device=self.dev)
                    for k, e in t["recv"].items()}
        # the fp32 image of every received bf16 message (the fused pass), guarded too
        self.dst32 = {k: torch.zeros(e.nbytes // 2 + GUARD, dtype=torch.int32, device=self.dev)
                      for k, e in t["recv"].items() if e.dtype == "bfloat16"}
        # the b messages of this case go through slot(): their producer (a GEMM with the identity) writes them
        self.direct = {k for k, e in t["send"].items() if name == "tiny_bf16_split" and k[0] == "b"}
        if self.direct:
            self.eye = torch.eye(D, dtype=BF16, device=self.dev)
        self.k = 0

    def _bits(self, step, key, sender, nbytes):
        if self.name == "tiny_bf16_split" and key[0] == "b":
            return finite_bf16(self.name, step, key[0], key[1], sender, nbytes // 2).view(torch.int32)
        return payload(self.name, step, key[0], key[1], sender, nbytes)

    def load(self, step):
        """Fresh payloads into the send tensors, sentinels into the destinations (before the step is issued)."""
        for k, e in self.pipe.table["send"].items():
            self.src[k].copy_(self._bits(step, k, self.rank, e.nbytes))
        for b in list(self.dst.values()) + list(self.dst32.values()):
            b.fill_(12345)

    def issue(self):
        from distributed_training_compare_jax_amd.ops.gemm import linear_into

        p = self.pipe
        p.begin_step()
        for it in self.prog:
            if it[0] == "post":
                for tag in it[3]:
                    if tag in self.direct:
                        linear_into(self.src[tag].view(BF16).view(-1, D), self.eye, p.slot(*tag))
                        p.send(tag[0], tag[1])
                    else:
                        p.send(tag[0], tag[1], self.src[tag])
            elif it[0] == "wait":
                for n in it[1]:
                    for tag in self.rcv[n]:
                        e = p.table["recv"][tag]
                        out = self.dst[tag][:e.nbytes // 4]
                        f32 = self.dst32[tag][:e.nbytes // 2].view(F32) if tag in self.dst32 else None
                        p.recv(tag[0], tag[1], out, f32)

    def verify(self, step, what):
        torch.cuda.synchronize()
        sent = torch.full((GUARD,), 12345, dtype=torch.int32)
        for k, e in self.pipe.table["recv"].items():
            exp = self._bits(step, k, self.rank + e.peer, e.nbytes)
            got = self.dst[k].cpu()
            nd = int((got != torch.cat([exp, sent])).sum())
            self.report(f"{self.name}/{what}/{k[0]}{k[1]}", nd == 0, nd)
            if k in self.dst32:
                got = self.dst32[k].cpu()
                nd = int((got != torch.cat([exp.view(BF16).float().view(torch.int32), sent])).sum())
                self.report(f"{self.name}/{what}/{k[0]}{k[1]}/f32", nd == 0, nd)
        self.pipe.check()
        self.report(f"{self.name}/{what}/check", True, 0)

    def skew(self):
        if self.k % self.W == self.rank:
            time.sleep(0.005)
        self.k += 1

    def run(self):
        for step in range(EAGER_STEPS):
            self.load(step)
            self.skew()
            self.issue()
            self.verify(step, f"eager{step}")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin(capture_error_mode="thread_local")
            self.issue()
            g.capture_end()
        torch.cuda.current_stream().wait_stream(s)
        for r in range(REPLAYS):
            step = EAGER_STEPS + r
            self.load(step)
            self.skew()
            g.replay()
            self.verify(step, f"replay{r}")
        assert int(self.pipe.epoch.item()) == EAGER_STEPS + REPLAYS  # the capture itself ran nothing
        self.pipe.close()


def _validation(d, report):
    """dtc_pp_send / dtc_pp_recv refuse misaligned and oversize arguments with 4001 and launch nothing."""
    import torch.distributed as dist

    from distributed_training_compare_jax_amd.ops import _native as N
    from distributed_training_compare_jax_amd.parallel.p2p import P2PPipe

    pipe = P2PPipe(dist.group.WORLD, d.rank, d.world, d.device, 1, False, {"f": (64, F32), "b": (64, F32)})
    L, st = N.lib(), N.stream_ptr(d.device)
    x = torch.zeros(128, dtype=torch.int32, device=d.device)
    own, peer = pipe._own, next(iter(pipe._peer.values()))
    ep, err, nb = pipe.epoch.data_ptr(), pipe.err.data_ptr(), pipe.bytes
    send = lambda x_, n, off, buf, flag: L.dtc_pp_send(x_, n, own, off, buf, peer, flag, ep, st)  # noqa: E731
    recv = lambda o, o32, n, off, buf, flag: L.dtc_pp_recv(o, o32, n, peer, off, buf, own, flag, ep, err, st)  # noqa: E731
    p = x.data_ptr()
    bad = {
        "send n%16": send(p, 24, 0, nb, 0),
        "send n<=0": send(p, 0, 0, nb, 0),
        "send offset%16": send(p, 16, 8, nb, 0),
        "send oversize": send(p, nb + 16, 0, nb, 0),
        "send offset+n>buf": send(p, 256, nb - 240, nb, 0),
        "send x%16": send(p + 4, 16, 0, nb, 0),
        "send flag<0": send(p, 16, 0, nb, -1),
        "send flag>=1024": send(p, 16, 0, nb, 1024),
        "recv n%16": recv(p, 0, 40, 0, nb, 0),
        "recv offset%16": recv(p, 0, 16, 4, nb, 0),
        "recv oversize": recv(p, 0, nb + 16, 0, nb, 0),
        "recv offset+n>buf": recv(p, 0, 256, nb - 240, nb, 0),
        "recv out%16": recv(p + 8, 0, 16, 0, nb, 0),
        "recv out_f32%16": recv(p, p + 260, 16, 0, nb, 0),
        "recv flag>=1024": recv(p, 0, 16, 0, nb, 1024),
    }
    torch.cuda.synchronize()
    for k, rc in bad.items():
        report(f"validation/{k}", rc == 4001, rc)
    report("validation/nothing_ran", int(pipe.epoch.item()) == 0 and int(pipe.err.item()) == 0, 0)
    # the host side names the stage and the message (a stage without that slot says so instead)
    for fn, match in ((lambda: pipe.send("f", 0, x[:7]), "its slot holds"), (lambda: pipe.send("s", 0, x), "has no send"),
                      (lambda: pipe.recv("b", 0, x[:5]), "the message is")):
        ok = False
        try:
            fn()
        except (RuntimeError, KeyError) as e:
            ok = f"stage {d.rank}" in str(e) and (match in str(e) or "has no" in str(e))
        report(f"validation/host/{match}", ok, 0)
    pipe.close()


def _worker(out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed

    d = init_distributed("cuda")
    torch.set_num_threads(max(1, 8 // d.world))
    reports = []
    path = os.path.join(out_dir, f"rank{d.rank}.json")

    def report(case, ok, ndiff):
        reports.append({"case": case, "ok": bool(ok), "ndiff": int(ndiff)})
        if not ok:
            with open(path, "w") as f:
                json.dump(reports, f)
            raise AssertionError(f"rank {d.rank}/{d.world} {case}: {ndiff}")

    for name, kind, M, hs, msgs in CASES:
        _Case(name, kind, M, hs, msgs, d, report).run()
    _validation(d, report)
    with open(path, "w") as f:
        json.dump(reports, f)
    destroy()


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("world", WORLDS)
def test_pp_messages_bitwise(cuda, world):
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
    for r, rep in enumerate(reps):
        names = [e["case"] for e in rep]
        assert len(names) == len(set(names))
        # every stage received something in every step of every case, the fused fp32 images included
        for name, _, _, _, _ in CASES:
            for what in [f"eager{k}" for k in range(EAGER_STEPS)] + [f"replay{k}" for k in range(REPLAYS)]:
                assert sum(n.startswith(f"{name}/{what}/") for n in names) >= 2, (r, name, what)
        assert any(n.endswith("/f32") for n in names) and sum(n.startswith("validation/") for n in names) == 19
