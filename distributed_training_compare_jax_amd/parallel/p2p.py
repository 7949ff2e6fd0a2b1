"""xGMI peer-to-peer all-reduce for tensor-parallel activations (``csrc/p2p.hip``).

SURVEY §2.3 / §5.8: TP makes 4 all-reduces of the fp32 residual ``[tokens, d_model]`` per
layer (+1 for the head).  On an 8×MI355X node every GPU has a direct xGMI link to every other
one; a ring all-reduce drives one outgoing link per step, while this two-shot kernel lets every
rank read its slice from all peers at once (reduce-scatter), then read every peer's reduced
slice (all-gather), through IPC-mapped peer buffers.

Being ordinary stream-ordered kernels (barriers are device-side epoch flags), the collective is
captured INTO the step's hipGraph: the TP step no longer cuts its graph at every all-reduce the
way an eager RCCL call does.  The sum runs in rank order on every rank, so TP replicas stay
bitwise identical (``tests/test_p2p_collectives_gpu.py`` pins every output bit at 2, 3, 5 and 8
ranks).  RCCL remains the path for anything else (non-fp32 all-reduces, oversize); scalars and
slots of fewer than 4 floats go through zero-padded vector elements (``parallel.tp.TPComm``).

Handles are exchanged once over the process group (``all_gather_object``), so the same code runs
on a real node (RCCL group) and in the one-GPU multi-process tests (gloo group, all ranks on one
device — IPC within a device works the same way).

Small messages (the vocab-parallel CE row statistics and label logits, the grad-norm scalar) take a
one-shot variant (one barrier; every rank sums all peers' buffers itself), so a TP step issues no
RCCL call at all: :class:`parallel.tp.TPComm` gathers by summing zero-padded slots.

:class:`P2PPipe` (below) carries the pipeline stages' point-to-point messages over the same kind of buffer
(``pp_comm: p2p``): sender-staged slots, epoch flags at the receiver, pulled by the receiver.
:class:`P2PGradReduce` carries a pure-DP step's gradient buckets, loss sum and embedding-gradient gather
(``dp_comm: p2p``); :class:`P2PZeroShard` the ZeRO-1 step's bucket reduce-scatters and parameter gathers
(``zero_comm: p2p``).
"""

from __future__ import annotations

import ctypes
import os

import torch
import torch.distributed as dist

from ..ops import _native as N


def _pci_bus_id(L, dev: int) -> str:
    buf = ctypes.create_string_buffer(64)
    N.check(L.dtc_device_pci_bus_id(dev, buf, 64), "hipDeviceGetPCIBusId")
    return buf.value.decode().lower()


def check_peer_access(L, rank: int, dev: int, peers, what: str = "P2P all-reduce", alt: str = "tp_comm: rccl") -> dict:
    """``peers``: [(rank, pci bus id)] of the group.  Every peer GPU must be reachable by direct
    loads from this one (hipDeviceCanAccessPeer over xGMI); raises naming the rank and peer
    otherwise — the P2P all-reduce never silently switches paths.  Peers on this same GPU (the
    one-GPU multi-process tests) need no peer access.  Returns {peer rank: "self" | "xgmi" |
    "not-visible"} (a peer GPU outside this process's visible set cannot be queried; its IPC
    mapping below still has to succeed)."""
    mine = _pci_bus_id(L, dev)
    n = ctypes.c_int(0)
    N.check(L.dtc_device_count(ctypes.byref(n)), "hipGetDeviceCount")
    ordinal = {_pci_bus_id(L, d): d for d in range(n.value)}
    out = {}
    for p, bus in peers:
        if p == rank:
            continue
        if bus == mine:
            out[p] = "self"
            continue
        if bus not in ordinal:
            out[p] = "not-visible"
            continue
        ok = ctypes.c_int(0)
        N.check(L.dtc_can_access_peer(dev, ordinal[bus], ctypes.byref(ok)), "hipDeviceCanAccessPeer")
        if not ok.value:
            raise RuntimeError(f"{what}: rank {rank} (GPU {dev}, {mine}) cannot access rank {p}'s GPU "
                               f"({bus}) directly; use {alt}")
        out[p] = "xgmi"
    return out


# error-word bases of the bounded waits in csrc/p2p.hip (ERR_BARRIER / ERR_FLAG / ERR_PP): a barrier's word is
# BARRIER_ERR + the rank waited for, a stream flag's FLAG_ERR + its index, a stage message's PP_ERR + its flag word
BARRIER_ERR, FLAG_ERR, PP_ERR = 1000, 2000, 3000


def barrier_timeout_message(label: str, unit: str, rank: int, e: int) -> str:
    """What a barrier's error word ``e`` says: ``label`` names the transport ("P2P all-reduce (PP group)"),
    ``unit`` what its members are called ("rank" or "stage"), ``rank`` is this member."""
    return f"{label}: {unit} {rank} timed out waiting for {unit} {e - BARRIER_ERR}"


class PeerBuffer:
    """This rank's uncached device buffer (flag area + ``nbytes`` of payload), exported over IPC, and the mapped
    buffers of its ``peers`` (default: every other rank of ``group``); the device epoch counter and error word of
    the kernels that use them.  One ``all_gather_object`` carries the handles, the PCI bus ids and, if given, a
    ``plan`` hash every rank must share (``plan_name``: what it hashes, for the message); one barrier ends the
    init.  ``label`` / ``unit`` / ``alt``: the transport's name in messages, "rank" or "stage", and the setting to
    recommend when a peer GPU cannot be reached."""

    def __init__(self, group, rank: int, world: int, device, nbytes: int, label: str, unit: str, alt: str,
                 peers=None, plan: str = None, plan_name: str = ""):
        self.rank, self.world, self.label, self.unit = rank, world, label, unit
        self.device = torch.device(device)
        L = N.lib()
        self._flag_bytes = int(L.dtc_p2p_flag_bytes())
        ptr = ctypes.c_void_p()
        handle = ctypes.create_string_buffer(64)
        with torch.cuda.device(self.device):
            N.check(L.dtc_p2p_alloc(self._flag_bytes + int(nbytes), ctypes.addressof(ptr), ctypes.addressof(handle)),
                    "dtc_p2p_alloc")
        self._own = ptr.value
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        info = [None] * world
        mine = (bytes(handle.raw), _pci_bus_id(L, dev)) + (() if plan is None else (plan,))
        dist.all_gather_object(info, mine, group=group)
        for p, other in enumerate(info):
            if plan is not None and other[2] != plan:
                raise RuntimeError(f"{label}: {unit} {rank} and {unit} {p} derived different {plan_name} "
                                   f"({plan[:12]} vs {other[2][:12]}): their configurations differ")
        peers = [p for p in (range(world) if peers is None else peers) if p != rank]
        self.peer_paths = check_peer_access(L, rank, dev, [(p, info[p][1]) for p in peers], what=label, alt=alt)
        self._mapped = {}  # peer -> its buffer's base as mapped here
        with torch.cuda.device(self.device):
            for p in peers:
                q = ctypes.c_void_p()
                hb = ctypes.create_string_buffer(info[p][0], 64)
                rc = L.dtc_p2p_open(ctypes.addressof(hb), ctypes.addressof(q))
                if rc != 0:
                    raise RuntimeError(f"{label}: {unit} {rank} could not map {unit} {p}'s buffer (GPU {info[p][1]}): "
                                       f"hipIpcOpenMemHandle error {rc}")
                self._mapped[p] = q.value
        self.epoch = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        # all ranks' flag areas are zero before anyone's first barrier or signal can run
        torch.cuda.synchronize(self.device)
        dist.barrier(group=group)

    def close(self):
        L = N.lib()
        for q in self._mapped.values():
            L.dtc_p2p_close(ctypes.c_void_p(q))
        self._mapped = {}
        if self._own:
            L.dtc_p2p_free(ctypes.c_void_p(self._own))
            self._own = None


class P2PAllReduce(PeerBuffer):
    def __init__(self, group, rank: int, world: int, device, max_bytes: int, label: str = "P2P all-reduce",
                 unit: str = "rank"):
        assert 1 <= world <= 8, "P2P all-reduce supports up to 8 ranks (one xGMI hive)"
        self.half = (int(max_bytes) + 4095) // 4096 * 4096
        super().__init__(group, rank, world, device, 2 * self.half, "P2P all-reduce", "rank", "tp_comm: rccl")
        self.label, self.unit = label, unit  # (of describe(); init and check() speak of "P2P all-reduce" ranks)
        bases = [self._own if p == rank else self._mapped[p] for p in range(world)]
        self._bases = (ctypes.c_void_p * 8)(*(bases + [None] * (8 - world)))
        self._bases_ptr = ctypes.addressof(self._bases)
        # what every native call on the object takes, in this order
        self._targs = (self._bases_ptr, rank, world, self.half, self.epoch.data_ptr(), self.err.data_ptr())
        # calls issued so far (host mirror of epoch / 2): the buffer half of the next call is calls & 1
        self.calls = 0

    def _call(self, name: str, head, *tail):
        """``name(*head, <bases, rank, world, half, epoch, err>, *tail)``, checked; one more call on the object."""
        N.check(getattr(N.lib(), name)(*head, *self._targs, *tail), name)
        self.calls += 1

    def supports(self, t: torch.Tensor) -> bool:
        return (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0
                and t.numel() * 4 <= self.half)

    def all_reduce_(self, t: torch.Tensor, mode: int = 0) -> torch.Tensor:
        """In-place sum over the group.  mode 0: one-shot (one barrier, every rank reads every peer) at
        W = 2 and for small messages (<= 1 MiB at W <= 4, <= 512 KiB at W >= 5), else two-shot (reduce-scatter
        + all-gather, 2 (W-1)/W of the bytes per rank); 1 / 2 force two-shot / one-shot."""
        self._call("dtc_p2p_allreduce", (t.data_ptr(), t.data_ptr(), t.numel()), int(mode), N.stream_ptr(t.device))
        return t

    def staged_out(self, numel: int, dtype=torch.bfloat16):
        """Where the producer of the NEXT call's bf16 payload should write it (this rank's buffer half
        of that call, a :class:`ops.gemm.RawOut`), or None if it does not fit.  The next call must then
        be :meth:`all_reduce_bf16` with ``x=None``.  The half is ``calls & 1``; :meth:`end_step` keeps
        the calls per step even so the half of each call site is the same on every graph replay."""
        from ..ops.gemm import RawOut

        esz = 2 if dtype == torch.bfloat16 else (4 if dtype == torch.float32 else 0)
        if not esz or numel % 8 or numel * esz > self.half:
            return None
        return RawOut(self._own + self._flag_bytes + (self.calls & 1) * self.half, dtype, self.device)

    def end_step(self):
        """Pad the step's calls to an even count with a payload-free barrier round (epoch + 2)."""
        if self.calls & 1:
            N.check(N.lib().dtc_p2p_barrier_round(*self._targs[:3], *self._targs[4:], N.stream_ptr(self.device)),
                    "dtc_p2p_barrier_round")  # (the one call that takes no half)
            self.calls += 1

    def supports_bf16(self, x: torch.Tensor) -> bool:
        return (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.numel() % 8 == 0
                and x.numel() * 2 <= self.half)

    def all_reduce_bf16(self, x, out: torch.Tensor, resid=None, bias=None, mode: int = 0) -> torch.Tensor:
        """out (fp32) = resid + bias + Σ_ranks x, x bf16 (the payload), fp32 sums in rank order; ``bias``
        indexed by the last dimension of ``out``.  Same barrier / buffer-half protocol as all_reduce_.
        ``x=None``: the payload (``out.numel()`` values) was written by its producer straight into
        :meth:`staged_out`, so no stage copy runs."""
        ncols = out.shape[-1] if bias is not None else 0
        n = out.numel() if x is None else x.numel()
        assert x is not None or n * 2 <= self.half
        self._call("dtc_p2p_allreduce_bf16", (N.ptr(x), out.data_ptr(), n), int(mode), N.ptr(resid), N.ptr(bias), ncols,
                   N.stream_ptr(out.device))
        return out

    # ---- sequence parallelism: row-sharded residual stream (parallel/tp.py TPComm.*_rows)
    def supports_rs(self, rows: int, cols: int, dtype) -> bool:
        esz = 2 if dtype == torch.bfloat16 else (4 if dtype == torch.float32 else 0)
        loc = rows // self.world * cols
        return bool(esz) and rows % self.world == 0 and loc % 8 == 0 and rows * cols * esz <= self.half

    def reduce_scatter(self, x, rows: int, cols: int, dtype, out: torch.Tensor, resid=None, bias=None) -> torch.Tensor:
        """out (fp32 [rows / W, cols], this rank's rows) = resid + bias + Σ_ranks x[own rows]; ``x`` the full
        [rows, cols] partial (bf16 / fp32) or None when its producer wrote it into :meth:`staged_out`."""
        if rows % self.world:  # rows // W would drop the last rows and shift every rank's slice
            raise RuntimeError(f"P2P reduce-scatter: {rows} rows do not divide over {self.world} ranks")
        n_loc = rows // self.world * cols
        self._call("dtc_p2p_reduce_scatter", (N.ptr(x), int(dtype == torch.bfloat16), out.data_ptr(), n_loc),
                   N.ptr(resid), N.ptr(bias), cols if bias is not None else 0, N.stream_ptr(out.device))
        return out

    def supports_ag(self, x: torch.Tensor) -> bool:
        nb = x.numel() * x.element_size()
        return x.is_cuda and x.is_contiguous() and nb % 16 == 0 and nb * self.world <= self.half

    def all_gather(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out [W * rows, ...] (rank-major) = every rank's ``x`` (any dtype, 16-byte multiple)."""
        self._call("dtc_p2p_all_gather", (x.data_ptr(), out.data_ptr(), x.numel() * x.element_size()),
                   N.stream_ptr(out.device))
        return out

    def check(self):
        """Raise if a barrier timed out (a peer never arrived); call at a host sync point.

        Also checks the buffer-half invariant :meth:`staged_out` relies on: every call advances the
        device epoch by 2, replays included, while the host counter only sees calls issued from Python
        (eager or captured), so the device half ``(epoch >> 1) & 1`` must equal the host half ``calls & 1``
        (true as long as every captured step is padded to an even count by :meth:`end_step`).  What this
        catches is a captured graph with an ODD call count: the host counts it once, every replay advances
        the epoch again, and after an even number of replays the two halves differ, so the next
        :meth:`staged_out` would point at the half the device does not reduce: raise instead.  An
        :meth:`end_step` alone does not repair that state (it advances both sides); one barrier round the
        host does not count (``dtc_p2p_barrier_round``), on every rank, does.  NOT caught: an eager call
        outside the step (eval, a debug all-reduce) without its own :meth:`end_step` advances host and
        device alike, so this check passes, yet the pointers a captured step got from :meth:`staged_out`
        are then one half off on replay.  Always pad out-of-step use with :meth:`end_step`
        (``Engine.evaluate`` does: its own program ends with one, eager and captured)."""
        e = int(self.err.item())
        if e:
            raise RuntimeError(barrier_timeout_message("P2P all-reduce", "rank", self.rank, e))
        dev_half = (int(self.epoch.item()) >> 1) & 1
        if dev_half != (self.calls & 1):
            raise RuntimeError(f"P2P all-reduce: rank {self.rank} buffer-half mismatch (device epoch "
                               f"{int(self.epoch.item())}, host calls {self.calls}): a captured graph with an odd "
                               "number of P2P calls was replayed; end every captured step with end_step()")

    def describe(self, e: int) -> str:
        """The message for this object's error word ``e`` under its ``label`` (which group) and ``unit``."""
        return barrier_timeout_message(self.label, self.unit, self.rank, e)


# ------------------------------------------------------------------------------ DP gradient buckets
# ``dp_comm: p2p`` (csrc/p2p.hip, "DP gradient buckets"): the bucket all-reduces of parallel/dp.py, the loss sum
# and the embedding-output gradient all-gather as stream-ordered kernels on ONE peer object.

# grid cap of the bucket kernels (blocks of 256 threads): they run under the backward GEMMs.  Chosen from the
# one-GPU A/B in profiles/dp_p2p.md (32 / 64 / 128 / 256: 14.13 / 12.3 / 11.68 / 11.60 ms per step); how many
# blocks saturate the xGMI links is unmeasured
DP_P2P_BLOCKS = 256


def dp_payload_bytes(numel: int, payload: str) -> int:
    """Bytes a bucket of ``numel`` fp32 grads takes in a buffer half: 16-byte pieces of 4 fp32 or 8 bf16
    values (the last bf16 piece zero-padded when numel % 8 == 4)."""
    return -(-int(numel) // 8) * 16 if payload == "bf16" else int(numel) * 4


def dp_half_bytes(buckets, payload: str, gather_bytes: int) -> int:
    """The buffer half that holds the largest bucket's payload, the gathered embedding-output gradients and
    the 4-float loss sum, rounded to 4096 like :class:`P2PAllReduce` does."""
    need = max([dp_payload_bytes(b - a, payload) for a, b in buckets] + [int(gather_bytes), 16])
    return (need + 4095) // 4096 * 4096


def dp_plan_hash(world: int, buckets, payload: str, half_bytes: int, gather_bytes: int) -> str:
    """What every rank of the DP group must agree on before it maps a peer: the bucket list, the payload
    dtype, the half size and the gather size."""
    import hashlib

    plan = (int(world), [(int(a), int(b)) for a, b in buckets], str(payload), int(half_bytes), int(gather_bytes))
    return hashlib.sha256(repr(plan).encode()).hexdigest()


class P2PGradReduce(P2PAllReduce):
    """The cross-process calls of a pure-DP step on one peer object (``TrainConfig.dp_comm: p2p``): the bucket
    all-reduces (:meth:`bucket_all_reduce_`), the loss sum (``all_reduce_`` of a 4-float buffer) and the
    embedding-output gradient ``all_gather``.  Nothing calls the process group after ``__init__``.

    Every call goes through :meth:`on_comm`, which runs it on ONE comm stream forked from the current stream
    (kernels only, so hipGraph capture records the fork), in the order the step issues them.  All cross-process
    waits of the group are then totally ordered and identical on every rank, whatever the runtime does with the
    graph's branches, and none sits on the main stream.  ``DTC_DP_P2P_STREAM=0``: no fork, the calls run in the
    issuing stream (serial; the A/B and the fallback)."""

    def __init__(self, group, rank: int, world: int, device, buckets, payload: str = "fp32", gather_bytes: int = 0,
                 max_blocks: int = None, use_stream: bool = None):
        if payload not in ("fp32", "bf16"):
            raise ValueError(f"P2P grad reduce: payload {payload!r}: expected 'fp32' or 'bf16'")
        if not 1 <= world <= 8:
            raise ValueError(f"P2P grad reduce: {world} ranks; supports up to 8 (one xGMI hive)")
        self.buckets = [(int(a), int(b)) for a, b in buckets]
        self.payload, self.gather_bytes = payload, int(gather_bytes)
        half, self.plan_hash = self._plan(world)
        seen = [None] * world
        dist.all_gather_object(seen, self.plan_hash, group=group)
        for p, h in enumerate(seen):
            if h != self.plan_hash:
                raise RuntimeError(f"P2P grad reduce: rank {rank} and rank {p} derived different bucket plans "
                                   f"({self.plan_hash[:12]} vs {h[:12]}): their configurations differ")
        super().__init__(group, rank, world, device, half, label="P2P all-reduce (DP group)")
        assert self.half == half
        if max_blocks is None:
            max_blocks = int(os.environ.get("DTC_DP_P2P_BLOCKS", str(DP_P2P_BLOCKS)))
        if not 1 <= int(max_blocks) <= 1024:
            raise ValueError(f"DTC_DP_P2P_BLOCKS={max_blocks}: expected 1 to 1024")
        self.max_blocks = int(max_blocks)
        if use_stream is None:
            use_stream = os.environ.get("DTC_DP_P2P_STREAM", "1") == "1"
        self._cs = torch.cuda.Stream(self.device) if use_stream else None
        self._held = []  # tensors the comm stream still reads (kept alive until join)

    def _plan(self, world: int):
        """(buffer half in bytes, the hash every rank must share)."""
        half = dp_half_bytes(self.buckets, self.payload, self.gather_bytes)
        return half, dp_plan_hash(world, self.buckets, self.payload, half, self.gather_bytes)

    def _bf(self, bf16) -> int:
        """The ``bf16`` argument of a bucket call: the object's payload unless the caller says otherwise."""
        return int(self.payload == "bf16" if bf16 is None else bool(bf16))

    def _blocks(self, max_blocks) -> int:
        return self.max_blocks if max_blocks is None else int(max_blocks)

    def bucket_all_reduce_(self, t: torch.Tensor, bf16: bool = None, max_blocks: int = None) -> torch.Tensor:
        """In-place sum of a slice of the flat fp32 grads over the group (``dtc_dp_allreduce``: pack, barrier,
        rank-order reduce of this rank's slice, barrier, gather; grids capped at ``max_blocks``)."""
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"P2P grad reduce: rank {self.rank} bucket is {tuple(t.shape)} {t.dtype} on {t.device}; "
                               "needs a contiguous fp32 GPU tensor")
        self._call("dtc_dp_allreduce", (t.data_ptr(), t.numel(), self._bf(bf16)), self._blocks(max_blocks),
                   N.stream_ptr(t.device))
        return t

    def on_comm(self, fn, keep=(), mark: bool = False):
        """Run ``fn`` (calls on this object) on the comm stream, after everything the current stream holds so
        far.  ``keep``: tensors ``fn`` reads that the caller may drop before :meth:`join`.  ``mark``: returns an
        event recorded behind ``fn`` for :meth:`wait_for` (None without a comm stream)."""
        if self._cs is None:
            fn()
            return None
        self._cs.wait_stream(torch.cuda.current_stream(self.device))
        ev = None
        with torch.cuda.stream(self._cs):
            fn()
            if mark:
                ev = torch.cuda.Event()
                ev.record(self._cs)
        self._held.extend(keep)
        return ev

    def wait_for(self, ev):
        """The current stream waits for a marked call (and the calls before it)."""
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def join(self):
        """The current stream waits for every call issued so far."""
        if self._cs is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._cs)
        self._held.clear()

    def close(self):
        self._held.clear()
        super().close()


# ------------------------------------------------------------------------------ ZeRO-1 over the DP buckets
# ``zero_comm: p2p`` (csrc/p2p.hip, "ZeRO-1 over the DP buckets"): the bucket all-reduce cut in the middle.  Each
# bucket is reduce-scattered under the backward, the sharded AdamW (train/optimizer.py P2PShardedAdamW) updates the
# owned slices, and a per-bucket gather moves the updated fp32 parameters and writes the bf16 mirror.

def zero_plan(buckets, world: int, payload: str):
    """Who owns what under ``zero_comm: p2p``: within a bucket ``[a, b)`` of ``n`` elements rank ``r`` owns the
    slice ``dp_reduce_kernel`` gives it -- 16-byte pieces of ``e`` = 4 (fp32 payload) or 8 (bf16) elements,
    ``chunk = ceil(pieces / W)``, pieces ``[min(pieces, r chunk), min(pieces, (r + 1) chunk))``, i.e. elements
    ``[a + min(n, e lo), a + min(n, e hi))``.  Trailing ranks may own a short or an empty slice; a bucket's slices are
    disjoint and cover it.

    Returns ``(ranges, offsets)``: ``ranges[r][i] = (lo, hi)`` is rank r's slice of bucket i (``lo == hi`` when
    empty), ``offsets[r][i]`` its start in the rank's compact m / v shard, and ``offsets[r][len(buckets)]`` the
    shard's length."""
    if payload not in ("fp32", "bf16"):
        raise ValueError(f"zero plan: payload {payload!r}: expected 'fp32' or 'bf16'")
    if not 1 <= int(world) <= 8:
        raise ValueError(f"zero plan: {world} ranks; supports 1 to 8")
    e = 8 if payload == "bf16" else 4
    ranges, offsets = [], []
    for r in range(int(world)):
        rr, oo, cur = [], [], 0
        for a, b in buckets:
            a, b = int(a), int(b)
            n = b - a
            if n <= 0 or n % 4 or a % 4:
                raise ValueError(f"zero plan: bucket [{a}, {b}) is not a positive multiple of 4 elements at a "
                                 "multiple of 4")
            pieces = -(-n // e)
            chunk = -(-pieces // world)
            lo = min(pieces, r * chunk)
            hi = min(pieces, lo + chunk)
            rr.append((a + min(n, e * lo), a + min(n, e * hi)))  # (an empty slice: lo == hi == pieces)
            oo.append(cur)
            cur += rr[-1][1] - rr[-1][0]
        oo.append(cur)
        ranges.append(rr)
        offsets.append(oo)
    return ranges, offsets


def zero_half_bytes(buckets, world: int, payload: str) -> int:
    """The buffer half that holds the larger of a bucket's gradient payload and a rank's fp32 parameter slice of
    that bucket (rank 0's is the largest; at world 1 with the bf16 payload the slice, the whole bucket in fp32, is
    twice the payload), and the 4-float sums; rounded to 4096."""
    ranges, _ = zero_plan(buckets, world, payload)
    need = 16
    for i, (a, b) in enumerate(buckets):
        need = max(need, dp_payload_bytes(b - a, payload), 4 * max(rr[i][1] - rr[i][0] for rr in ranges))
    return (need + 4095) // 4096 * 4096


def zero_plan_hash(world: int, buckets, payload: str, half_bytes: int) -> str:
    """What every rank of the DP group must agree on before it maps a peer, and what a checkpoint's Adam shards
    were cut by: the bucket list, the world, the payload (it sets the piece size of the ownership) and the half."""
    import hashlib

    ranges, offsets = zero_plan(buckets, world, payload)
    plan = ("zero1", int(world), [(int(a), int(b)) for a, b in buckets], str(payload), int(half_bytes), ranges,
            offsets)
    return hashlib.sha256(repr(plan).encode()).hexdigest()


def dp_rs_slots(numel: int, payload: str, world: int, max_blocks: int) -> int:
    """Blocks of a bucket's reduce-scatter = its per-block partial slots (csrc/p2p.hip dtc_dp_rs_slots)."""
    pieces = -(-int(numel) // 8) if payload == "bf16" else int(numel) // 4
    chunk = -(-pieces // int(world))
    return min(int(max_blocks), max(1, (chunk + 255) // 256))


class P2PZeroShard(P2PGradReduce):
    """The cross-process calls of a ZeRO-1 step on one peer object (``TrainConfig.zero_comm: p2p``): per bucket a
    reduce-scatter under the backward (:meth:`bucket_reduce_scatter_`) and, after the sharded update, a parameter
    gather (:meth:`bucket_param_gather_`); the loss sum and the global sum of squares go through ``all_reduce_`` of
    a 4-float buffer.  Calls are issued through :meth:`on_comm` like the all-reduce buckets: the one-barrier
    argument of the kernels needs all of them in one stream order."""

    def __init__(self, group, rank: int, world: int, device, buckets, payload: str = "fp32", max_blocks: int = None,
                 use_stream: bool = None):
        super().__init__(group, rank, world, device, buckets, payload, 0, max_blocks, use_stream)
        self.ranges, self.offsets = zero_plan(self.buckets, world, payload)
        self.owned = self.ranges[rank]

    def _plan(self, world: int):
        half = zero_half_bytes(self.buckets, world, self.payload)
        return half, zero_plan_hash(world, self.buckets, self.payload, half)

    def rs_slots(self, numel: int, bf16: bool = None, max_blocks: int = None) -> int:
        return dp_rs_slots(numel, "bf16" if self._bf(bf16) else "fp32", self.world, self._blocks(max_blocks))

    def bucket_reduce_scatter_(self, t: torch.Tensor, part: torch.Tensor, bf16: bool = None,
                               max_blocks: int = None) -> torch.Tensor:
        """``t`` (a bucket of the flat fp32 grads): this rank's slice of it becomes the rank-ordered sum over the
        group, in place, the rest of ``t`` is left as it is; ``part`` (fp32, :meth:`rs_slots` elements) gets the
        slice's per-block partial sums of squares."""
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and part.is_cuda
                and part.dtype == torch.float32 and part.is_contiguous()):
            raise RuntimeError(f"P2P zero shard: rank {self.rank} bucket is {tuple(t.shape)} {t.dtype} on {t.device}; "
                               "needs contiguous fp32 GPU tensors")
        self._call("dtc_dp_reduce_scatter", (t.data_ptr(), t.numel(), self._bf(bf16), part.data_ptr(), part.numel()),
                   self._blocks(max_blocks), N.stream_ptr(t.device))
        return t

    def bucket_param_gather_(self, p: torch.Tensor, mirror=None, n_mirror: int = 0, bf16: bool = None,
                             max_blocks: int = 1024) -> torch.Tensor:
        """``p`` (a bucket of the flat fp32 params, this rank's slice of it updated): every other rank's slice is
        pulled from its owner; ``mirror[:n_mirror]`` (bf16, the bucket's part of the compute mirror) is written
        from the same values in the same pass.  ``bf16`` selects the ownership plan (that of the gradient
        payload); the parameters travel as fp32."""
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError(f"P2P zero shard: rank {self.rank} bucket is {tuple(p.shape)} {p.dtype} on {p.device}; "
                               "needs a contiguous fp32 GPU tensor")
        if n_mirror and not (mirror is not None and mirror.dtype == torch.bfloat16 and mirror.is_contiguous()
                             and mirror.numel() >= n_mirror):
            raise RuntimeError(f"P2P zero shard: rank {self.rank} mirror of {n_mirror} elements needs a contiguous "
                               "bf16 tensor at least that long")
        self._call("dtc_dp_param_gather", (p.data_ptr(), N.ptr(mirror) if n_mirror else None, p.numel(), int(n_mirror),
                                           self._bf(bf16)), int(max_blocks), N.stream_ptr(p.device))
        return p


# ------------------------------------------------------------------------------ pipeline stage messages
# ``pp_comm: p2p`` (csrc/p2p.hip, "pipeline stage messages"): the f / b / s messages of parallel/pp.py as
# stream-ordered kernels.  The sender stages a message into a slot of its OWN buffer and stores the step
# epoch into a flag word of the receiver's buffer; the receiver waits on that word and pulls the slot.

PP_SLOT_ALIGN = 256
FLAG_WORDS = 1024  # csrc/p2p.hip FLAG_BYTES / 4


class PPSlot(tuple):
    """(peer, offset, nbytes, flag, buf_bytes, dtype name): ``peer`` = +1 / -1 (the next / previous stage);
    ``offset`` = payload offset of the slot in the SENDER's buffer; ``flag`` = word index in the RECEIVER's flag
    area; ``buf_bytes`` = payload bytes of the sender's buffer.  The same values on both ends of a message."""

    __slots__ = ()
    peer = property(lambda self: self[0])
    offset = property(lambda self: self[1])
    nbytes = property(lambda self: self[2])
    flag = property(lambda self: self[3])
    buf_bytes = property(lambda self: self[4])
    dtype = property(lambda self: self[5])


def _esize(dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def pp_slot_table(S: int, M: int, head_split: bool, msgs) -> list:
    """The slot and flag layout of every stage, a pure function of (S, M, head split, message shapes and
    dtypes), so every rank derives the same table (:class:`P2PPipe` exchanges its hash at init).

    ``msgs``: {"f": (numel, dtype), "b": (numel, dtype)} plus, with the head split, "fh" (the final LayerNorm
    output, the f message between the last two stages) and "s" (the packed row statistics, both ways).
    One slot and one flag word per (direction, kind, microbatch).  Stage s's buffer holds its outgoing slots:
    first those to s + 1 (f(0..M-1), then s(0..M-1) on stage S - 2 of a split head), then those to s - 1
    (b(0..M-1), then s(0..M-1) on stage S - 1 of a split head), each aligned to 256 bytes.  Its flag words
    count its incoming messages in the same order: from s - 1 first, then from s + 1.

    Returns ``table[s] = {"send": {(kind, i): PPSlot}, "recv": {(kind, i): PPSlot}, "bytes": payload bytes,
    "flags": flag words used}``; raises ValueError on a message that is not a multiple of 16 bytes or when a
    stage needs more flag words than the 4096-byte flag area holds."""
    if S < 2 or M < 1:
        raise ValueError(f"P2P pipe: needs at least 2 stages and 1 microbatch (S={S}, M={M})")

    def size(kind, a):  # message `kind` between stages a and a + 1
        key = "fh" if (kind == "f" and head_split and a == S - 2) else kind
        if key not in msgs:
            raise ValueError(f"P2P pipe: no shape given for message kind {key!r}")
        numel, dtype = msgs[key]
        nb = int(numel) * _esize(dtype)
        if nb <= 0 or nb % 16:
            raise ValueError(f"P2P pipe: message {key!r} ({numel} x {dtype}) is {nb} bytes, not a positive multiple "
                             "of 16 (the copy kernels move 16-byte pieces)")
        return nb, str(dtype).replace("torch.", "")

    out_up, out_dn = [], []  # per stage: [(kind, i, nbytes, dtype)] to s + 1 / to s - 1
    for s in range(S):
        up, dn = [], []
        if s < S - 1:
            up += [("f", i) + size("f", s) for i in range(M)]
            if head_split and s == S - 2:
                up += [("s", i) + size("s", s) for i in range(M)]
        if s > 0:
            dn += [("b", i) + size("b", s - 1) for i in range(M)]
            if head_split and s == S - 1:
                dn += [("s", i) + size("s", s - 1) for i in range(M)]
        out_up.append(up)
        out_dn.append(dn)
    offs, total = [], []
    for s in range(S):
        o, cur = {}, 0
        for d, lst in ((+1, out_up[s]), (-1, out_dn[s])):
            for kind, i, nb, _ in lst:
                o[(d, kind, i)] = cur
                cur += (nb + PP_SLOT_ALIGN - 1) // PP_SLOT_ALIGN * PP_SLOT_ALIGN
        offs.append(o)
        total.append(cur)
    table = [{"send": {}, "recv": {}, "bytes": total[s], "flags": 0} for s in range(S)]
    for r in range(S):  # receiver r: flags for the messages from r - 1 (their "up" list), then from r + 1
        k = 0
        for src, d, lst in ((r - 1, +1, out_up[r - 1] if r > 0 else []), (r + 1, -1, out_dn[r + 1] if r + 1 < S else [])):
            for kind, i, nb, dt in lst:
                table[src]["send"][(kind, i)] = PPSlot((d, offs[src][(d, kind, i)], nb, k, total[src], dt))
                table[r]["recv"][(kind, i)] = PPSlot((-d, offs[src][(d, kind, i)], nb, k, total[src], dt))
                k += 1
        if k > FLAG_WORDS:
            raise ValueError(f"P2P pipe: stage {r} needs {k} flag words (one per direction, message kind and "
                             f"microbatch; M={M}), the flag area holds {FLAG_WORDS}")
        table[r]["flags"] = k
    return table


def pp_table_hash(S: int, M: int, head_split: bool, table) -> str:
    import hashlib

    rows = [(s, kind, sorted((k, tuple(v)) for k, v in t[kind].items())) for s, t in enumerate(table)
            for kind in ("send", "recv")]
    return hashlib.sha256(repr((S, M, bool(head_split), rows, [t["bytes"] for t in table])).encode()).hexdigest()


class P2PPipe(PeerBuffer):
    """The pipeline stage messages of one PP group as in-graph kernels (``TrainConfig.pp_comm: p2p``).

    ``send`` / ``recv`` enqueue kernels on the current stream and return at once: nothing here calls the process
    group after ``__init__``, so hipGraph capture records a stage's whole step, messages included.  The flag a
    receive waits for carries the STEP EPOCH, a device counter :meth:`begin_step` bumps once per step (eager or
    replayed), so all stages count steps alike with no host involvement.  A slot is rewritten one step after
    it was read; that the schedule orders the rewrite after the read is what
    ``parallel.pp.check_slot_reuse`` proves for every supported (schedule, S, M)."""

    def __init__(self, group, stage: int, n_stages: int, device, n_micro: int, head_split: bool, msgs):
        if not 2 <= n_stages <= 8:
            raise ValueError(f"P2P pipe: {n_stages} stages; supports 2 to 8 (one xGMI hive)")
        full = pp_slot_table(n_stages, n_micro, head_split, msgs)
        self.table = full[stage]
        self._hash = pp_table_hash(n_stages, n_micro, head_split, full)
        self.bytes = self.table["bytes"]
        near = [p for p in (stage - 1, stage + 1) if 0 <= p < n_stages]
        super().__init__(group, stage, n_stages, device, max(self.bytes, 4096), "P2P pipe", "stage", "pp_comm: rccl",
                         peers=near, plan=self._hash, plan_name="slot tables")
        assert self._flag_bytes == 4 * FLAG_WORDS
        self._peer = {p - stage: q for p, q in self._mapped.items()}  # +1 / -1 -> the neighbour's buffer
        self._flag_names = {v.flag: (k, v.peer) for k, v in self.table["recv"].items()}

    def begin_step(self):
        """Bump the step epoch; once per step, inside the step (so a replayed graph bumps it too)."""
        N.check(N.lib().dtc_epoch_inc(self.epoch.data_ptr(), N.stream_ptr(self.device)), "dtc_epoch_inc")

    def _entry(self, which, tag, i):
        try:
            return self.table[which][(tag, i)]
        except KeyError:
            raise KeyError(f"P2P pipe: stage {self.rank} has no {which} slot for message ({tag!r}, {i})") from None

    def slot(self, tag: str, i: int):
        """This stage's outgoing slot of message (tag, i) (an ``ops.gemm.RawOut``) for a producer that writes
        it directly; :meth:`send` is then called with ``x=None``."""
        from ..ops.gemm import RawOut

        e = self._entry("send", tag, i)
        return RawOut(self._own + self._flag_bytes + e.offset, getattr(torch, e.dtype), self.device)

    def send(self, tag: str, i: int, x=None):
        """Stage ``x`` (or nothing: the producer wrote :meth:`slot`) and signal the receiver.  Never waits."""
        e = self._entry("send", tag, i)
        if x is not None and (not x.is_contiguous() or x.numel() * x.element_size() != e.nbytes):
            raise RuntimeError(f"P2P pipe: stage {self.rank} message ({tag!r}, {i}) is {tuple(x.shape)} {x.dtype}, "
                               f"its slot holds {e.nbytes} contiguous bytes")
        N.check(N.lib().dtc_pp_send(N.ptr(x), e.nbytes, self._own, e.offset, e.buf_bytes, self._peer[e.peer], e.flag,
                                    self.epoch.data_ptr(), N.stream_ptr(self.device)), "dtc_pp_send")

    def recv(self, tag: str, i: int, out: torch.Tensor, out_f32=None):
        """Wait for this step's message (tag, i) and copy it into ``out``; ``out_f32``: also the fp32 image of
        a bf16 message (exact), in the same pass."""
        e = self._entry("recv", tag, i)
        if not out.is_contiguous() or out.numel() * out.element_size() != e.nbytes:
            raise RuntimeError(f"P2P pipe: stage {self.rank} destination of ({tag!r}, {i}) is {tuple(out.shape)} "
                               f"{out.dtype}, the message is {e.nbytes} contiguous bytes")
        if out_f32 is not None and (e.dtype != "bfloat16" or out_f32.dtype != torch.float32
                                    or not out_f32.is_contiguous() or out_f32.numel() * 2 != e.nbytes):
            raise RuntimeError(f"P2P pipe: stage {self.rank} fp32 image of ({tag!r}, {i}): needs a bf16 message and "
                               f"a contiguous fp32 tensor of {e.nbytes // 2} elements")
        N.check(N.lib().dtc_pp_recv(out.data_ptr(), N.ptr(out_f32), e.nbytes, self._peer[e.peer], e.offset,
                                    e.buf_bytes, self._own, e.flag, self.epoch.data_ptr(), self.err.data_ptr(),
                                    N.stream_ptr(self.device)), "dtc_pp_recv")

    def describe(self, e: int) -> str:
        (tag, i), peer = self._flag_names.get(e - PP_ERR, (("?", -1), 0))
        return (f"P2P pipe: stage {self.rank} timed out waiting for flag {e - PP_ERR} (message ({tag!r}, {i}) from "
                f"stage {self.rank + peer})")

    def check(self):
        """Raise if a receive timed out (its sender never signalled); call at a host sync point."""
        e = int(self.err.item())
        if e:
            raise RuntimeError(self.describe(e))
