"""``dp_comm: p2p`` without a GPU: the configurations the schema and the engine refuse, the unchanged ``rccl``
buckets, the plan hash the ranks exchange at init, and self-checks of the torch emulations the GPU test
(tests/test_dp_p2p_gpu.py) compares every output bit against.

The emulations are written from the formulas in the ``csrc/p2p.hip`` header ("DP gradient buckets"), from no kernel
output: fp32 ``s = x[0]; s = s + x[p]`` in rank order; bf16 ``a = 0; a += float(bf16(x[p]))`` in rank order, one
rounding to bf16, widened exactly.
"""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.parallel.dp import GradBuckets
from distributed_training_compare_jax_amd.parallel.p2p import dp_half_bytes, dp_payload_bytes, dp_plan_hash

from test_dp_p2p_gpu import emu_bucket, inputs, slice_bounds

BF16, F32 = torch.bfloat16, torch.float32


def _tc(**kw):
    return TrainConfig(seed=0, parallel=kw.pop("parallel", "dp"), batch=kw.pop("batch", 8), steps=1, log_every=1000,
                       output_dir="/tmp/unused", **kw)


def _engine(tc, world, device):
    from distributed_training_compare_jax_amd.train.engine import Engine

    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    return Engine(mc, tc, OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, world, 0, torch.device(device), "gloo"))


# ------------------------------------------------------------------------------------------------ schema / engine

def test_dp_comm_defaults_to_rccl():
    assert _tc().dp_comm == "rccl"
    assert TrainConfig.__dataclass_fields__["dp_comm"].default == "rccl"


def test_engine_rejects_unknown_dp_comm():
    for bad in ("auto", "nccl", ""):
        with pytest.raises(ValueError, match="dp_comm"):
            _engine(_tc(dp_comm=bad, device="cpu"), 1, "cpu")


@pytest.mark.parametrize("what,tc_kw,world,device", [
    ("CPU device", dict(), 2, "cpu"),
    ("tp=2", dict(dp=2, tp=2), 4, "cuda"),
    ("pp=2", dict(dp=2, pp=2, pp_microbatches=2), 4, "cuda"),
    ("zero_stage=1", dict(zero_stage=1), 2, "cuda"),
    ("dp=16", dict(batch=16), 16, "cuda"),
    ("dp == 1", dict(), 1, "cuda"),
])
def test_engine_refuses_unsupported_p2p_layouts(what, tc_kw, world, device):
    """Raised before the engine touches the device or the process group (none exists here)."""
    with pytest.raises(ValueError, match="dp_comm: p2p cannot be combined with .*" + what):
        _engine(_tc(dp_comm="p2p", **tc_kw), world, device)


def test_rehearsal_at_dp1_needs_a_process_group():
    with pytest.raises(ValueError, match="dp_comm: p2p cannot be combined with .*process group"):
        _engine(_tc(dp_comm="p2p", dp_comm_rehearsal=True), 1, "cuda")


def test_rccl_builds_todays_buckets():
    """``dp_comm: rccl`` (the default): the engine's GradBuckets is what the constructor builds without the new
    arguments -- same buckets, the process-group transport, no peer object."""
    eng = _engine(_tc(device="cpu", dp_bucket_mb=0.25, dp_tail_mb=0.05), 1, "cpu")
    bk = eng.buckets
    assert eng.dp_p2p is None and bk.transport == "rccl" and bk.peer is None
    assert eng.loss.numel() == 1 and eng.loss.untyped_storage().nbytes() == 4
    ref = GradBuckets(eng.flat, None, 1, eng.program, 0.25, tail_mb=0.05, boundaries=None)
    assert ref.transport == "rccl" and ref.peer is None
    names = list(eng.flat.slots)
    ends = [eng.flat.range_of([n for n in names if n.startswith(f"h.{l}.")])[1] for l in eng.layout.layers]
    head = [n for n in names if n.startswith("lm_head") or n.startswith("lnf")]
    same = GradBuckets(eng.flat, None, 1, eng.program, 0.25, tail_mb=0.05,
                       boundaries=ends + [eng.flat.range_of(head)[1]])
    assert same.buckets == bk.buckets and len(bk.buckets) >= 3
    # an active rccl bucket goes through program.comm, as before
    calls = []

    class _Prog:
        def comm(self, fn, name=None, sig=None, capturable=True):
            calls.append(name)

    act = GradBuckets(eng.flat, None, 2, _Prog(), 0.25, tail_mb=0.05, active=True)
    act.ready_all()
    assert calls == [f"dp_bucket{i}" for i in range(len(act.buckets))]
    with pytest.raises(ValueError, match="dp_comm"):
        GradBuckets(eng.flat, None, 2, _Prog(), transport="auto")


def test_p2p_buckets_go_to_the_peer_in_issue_order():
    """transport="p2p": ``_issue`` hands the bucket's view to the peer's comm stream, ``wait_all`` joins it; the
    program sees no collective."""
    eng = _engine(_tc(device="cpu", dp_bucket_mb=0.25, dp_tail_mb=0.05), 1, "cpu")
    log = []

    class _Peer:
        def on_comm(self, fn, keep=(), mark=False):
            fn()

        def bucket_all_reduce_(self, view):
            log.append((view.data_ptr(), view.numel()))

        def join(self):
            log.append("join")

    class _NoProg:
        def comm(self, *a, **k):
            raise AssertionError("p2p transport issued a process-group collective")

        wait = comm

    bk = GradBuckets(eng.flat, None, 2, _NoProg(), 0.25, tail_mb=0.05, active=True, transport="p2p", peer=_Peer())
    bk.ready_upto(bk.buckets[0][1])
    assert log == [(eng.flat.grads[0:].data_ptr(), bk.buckets[0][1])]
    bk.ready_all()
    bk.wait_all()
    base = eng.flat.grads.data_ptr()
    assert log == [(base + 4 * a, b - a) for a, b in bk.buckets] + ["join"]
    assert bk.issued == [False] * len(bk.buckets)


# ------------------------------------------------------------------------------------------------ plan

def test_plan_hash_depends_on_every_input():
    bks = [(0, 40000), (40000, 65536), (65536, 70004)]
    half = dp_half_bytes(bks, "fp32", 1 << 16)
    h = dp_plan_hash(2, bks, "fp32", half, 1 << 16)
    assert h == dp_plan_hash(2, list(bks), "fp32", half, 1 << 16)
    assert h != dp_plan_hash(2, [(0, 40004), (40004, 65536), (65536, 70004)], "fp32", half, 1 << 16)  # a bucket size
    assert h != dp_plan_hash(2, bks, "bf16", half, 1 << 16)                                           # the payload
    assert h != dp_plan_hash(2, bks, "fp32", half + 4096, 1 << 16)
    assert h != dp_plan_hash(2, bks, "fp32", half, 1 << 15)
    assert h != dp_plan_hash(4, bks, "fp32", half, 1 << 16)


def test_half_holds_the_largest_payload_and_the_gather():
    assert dp_payload_bytes(4, "bf16") == 16 and dp_payload_bytes(12, "bf16") == 32 and dp_payload_bytes(12, "fp32") == 48
    bks = [(0, 40000), (40000, 65540)]
    assert dp_half_bytes(bks, "fp32", 0) == 160000 // 4096 * 4096 + 4096
    assert dp_half_bytes(bks, "bf16", 0) == 81920  # 40000 * 2 = 80000 -> the next multiple of 4096
    assert dp_half_bytes(bks, "bf16", 1 << 20) == 1 << 20
    assert dp_half_bytes([(0, 4)], "bf16", 0) == 4096
    # the padded last piece of n % 8 == 4 fits wherever n * 2 bytes do: the half is a multiple of 16
    for n in (4, 2044, 2048, 2052):
        assert dp_payload_bytes(n, "bf16") <= (n * 2 + 4095) // 4096 * 4096


# ------------------------------------------------------------------------------------------------ emulations

@pytest.mark.parametrize("W", (2, 3, 5, 8))
def test_selfcheck_emulations(W):
    n = 8 * 1031 + 4
    xs = inputs(("self", W), n, W)
    assert all(x.dtype == F32 and x.numel() == n for x in xs)
    assert not torch.equal(xs[0], xs[1]) and not torch.equal(xs[0], inputs(("self", W, 1), n, W)[0])
    ref = sum(x.double() for x in xs)
    mag = sum(x.double().abs() for x in xs)
    f = emu_bucket(xs, False)
    assert f.dtype == F32 and bool(((f.double() - ref).abs() <= W * 2.0 ** -24 * mag).all())
    s = xs[0].clone()
    for x in xs[1:]:
        s = s + x
    assert torch.equal(f, s)
    b = emu_bucket(xs, True)
    assert b.dtype == F32 and torch.equal(b, b.to(BF16).float())  # exactly bf16 values, widened
    a = torch.zeros(n)
    for x in xs:
        a = a + x.to(BF16).float()
    assert torch.equal(b, a.to(BF16).float())
    # bf16 keeps 8 significant bits: the payload rounding moves an input by at most half an ulp <= 2^-8 |x|, the one
    # rounding of the sum by half a bf16 ulp of a, and the fp32 adds by W 2^-24 of the magnitudes
    half_ulp = torch.ldexp(torch.ones(n, dtype=torch.float64), torch.frexp(a)[1] - 9)
    assert bool(((b.double() - ref).abs() <= half_ulp + (2.0 ** -8 + W * 2.0 ** -24) * mag).all())
    if W >= 3:  # a bitwise pass says something about the order
        assert int((emu_bucket(xs[::-1], False) != f).sum()) >= 0.05 * n
    assert int((emu_bucket(xs[:-1], False) != f).sum()) > 0.9 * n   # a dropped rank
    assert int((b != f).sum()) > 0.9 * n                            # which payload ran is visible


@pytest.mark.parametrize("W", (2, 3, 5, 8))
def test_selfcheck_slice_bounds(W):
    """chunk = ceil(pieces / W): the slices tile [0, pieces); trailing ranks may own a short or an empty one."""
    for pieces in (1, 2, W - 1, W, W + 1, 2 * W - 1, 2 * W + 1, 1031):
        if pieces < 1:
            continue
        b = [slice_bounds(pieces, W, r) for r in range(W)]
        assert b[0][0] == 0 and all(lo <= hi for lo, hi in b)
        covered = [i for lo, hi in b for i in range(lo, hi)]
        assert covered == list(range(pieces))
    assert slice_bounds(1, W, W - 1) == (1, 1)  # 4 elements in bf16 mode: one piece, every other rank owns nothing


# ------------------------------------------------------------------------------------------------ timeout messages

def test_barrier_timeout_messages_and_error_bases():
    """The pure decoder of a barrier's error word gives the three all-reduce messages the engine raises, and the
    error bases are the ones the kernels store (csrc/p2p.hip)."""
    import os
    import re

    from distributed_training_compare_jax_amd.parallel import p2p

    assert (p2p.BARRIER_ERR, p2p.FLAG_ERR, p2p.PP_ERR) == (1000, 2000, 3000)
    msg = p2p.barrier_timeout_message
    assert msg("P2P all-reduce", "rank", 1, 1003) == "P2P all-reduce: rank 1 timed out waiting for rank 3"
    assert msg("P2P all-reduce (PP group)", "stage", 0, 1001) == \
        "P2P all-reduce (PP group): stage 0 timed out waiting for stage 1"
    assert msg("P2P all-reduce (DP group)", "rank", 7, 1000) == \
        "P2P all-reduce (DP group): rank 7 timed out waiting for rank 0"
    src = open(os.path.join(os.path.dirname(p2p.__file__), "..", "csrc", "p2p.hip")).read()
    dev = re.search(r"ERR_BARRIER = (\d+), ERR_FLAG = (\d+), ERR_PP = (\d+);", src)
    assert dev and tuple(map(int, dev.groups())) == (1000, 2000, 3000)
