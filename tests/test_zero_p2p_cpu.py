"""``zero_comm: p2p`` without a GPU: the default, the configurations the engine refuses, the unchanged ``rccl`` ZeRO-1
class, the ownership plan (``parallel.p2p.zero_plan``) and its hash, and self-checks of the torch emulations the GPU
test (tests/test_zero_p2p_gpu.py) compares every output bit against.

The plan is checked against ``slice_bounds`` of tests/test_dp_p2p_gpu.py, which restates the slice of
``dp_reduce_kernel`` (chunk = ceil(pieces / W)) and was written from the ``csrc/p2p.hip`` header, not from this plan.
"""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, build_configs
from distributed_training_compare_jax_amd.parallel.p2p import (dp_payload_bytes, dp_rs_slots, zero_half_bytes, zero_plan,
                                                               zero_plan_hash)

from test_dp_p2p_cpu import _engine, _tc
from test_dp_p2p_gpu import emu_bucket, inputs, slice_bounds
from test_zero_p2p_gpu import emu_gather, emu_mirror, emu_scatter, owned, sumsq_bound

BF16, F32 = torch.bfloat16, torch.float32
WORLDS = (1, 2, 3, 5, 8)


def bucket_sizes(W):
    return [4, 8, 8 * W - 4, 8 * W + 4, 4 * 1031, 8 * 1031, 40004]


def tiled(ns, start=0):
    out, a = [], start
    for n in ns:
        out.append((a, a + n))
        a += n
    return out


# ------------------------------------------------------------------------------------------------ schema / engine

def test_zero_comm_defaults_to_rccl():
    assert _tc().zero_comm == "rccl"
    assert TrainConfig.__dataclass_fields__["zero_comm"].default == "rccl"
    assert build_configs("configs/train_config_dp_zero1.yaml")[0].zero_comm == "rccl"
    tc = build_configs("configs/train_config_dp_zero1_p2p.yaml")[0]
    assert (tc.zero_comm, tc.zero_stage, tc.dp_comm) == ("p2p", 1, "rccl")


def test_engine_rejects_unknown_zero_comm():
    for bad in ("auto", "nccl", ""):
        with pytest.raises(ValueError, match="zero_comm"):
            _engine(_tc(zero_comm=bad, zero_stage=1, device="cpu"), 1, "cpu")


@pytest.mark.parametrize("what,tc_kw,world,device", [
    ("zero_stage=0", dict(zero_stage=0), 2, "cuda"),
    ("CPU device", dict(zero_stage=1), 2, "cpu"),
    ("tp=2", dict(zero_stage=1, dp=2, tp=2), 4, "cuda"),
    ("pp=2", dict(zero_stage=1, dp=2, pp=2, pp_microbatches=2), 4, "cuda"),
    ("dp=16", dict(zero_stage=1, batch=16), 16, "cuda"),
    ("dp == 1", dict(zero_stage=1), 1, "cuda"),
    ("process group", dict(zero_stage=1, dp_comm_rehearsal=True), 1, "cuda"),
    ("dp_comm: p2p", dict(zero_stage=1, dp_comm="p2p"), 2, "cuda"),
])
def test_engine_refuses_unsupported_zero_p2p_layouts(what, tc_kw, world, device):
    """Raised before the engine touches the device or the process group (none exists here)."""
    with pytest.raises(ValueError, match="zero_comm: p2p cannot be combined with .*" + what):
        _engine(_tc(zero_comm="p2p", **tc_kw), world, device)


def test_dp_comm_p2p_still_refuses_zero_stage_1():
    with pytest.raises(ValueError, match="dp_comm: p2p cannot be combined with .*zero_stage=1.*zero_comm: p2p"):
        _engine(_tc(dp_comm="p2p", zero_stage=1), 2, "cuda")


def test_rccl_zero_builds_todays_sharded_adamw(monkeypatch):
    """``zero_comm: rccl`` + ``zero_stage: 1``: the class, its shard bounds and the call sequence are today's -- one
    collective on the whole flat gradient, the tail's and the norm's all-reduce, one gather of the parameters, all
    through ``program.comm``, then ``refresh_mirror``; no bucket is issued and no peer object exists."""
    from distributed_training_compare_jax_amd.config.schema import model_config_from_preset
    from distributed_training_compare_jax_amd.parallel.dist import DistInfo
    from distributed_training_compare_jax_amd.train.engine import Engine
    from distributed_training_compare_jax_amd.train.optimizer import P2PShardedAdamW, ShardedAdamW

    # a dp2 engine on the CPU without a process group: nothing collective runs at construction
    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    eng = Engine(mc, _tc(zero_stage=1, device="cpu", dp_bucket_mb=0.25, dp_tail_mb=0.05),
                 OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 2, 0, torch.device("cpu"), "gloo"))
    opt = eng.opt
    assert type(opt) is ShardedAdamW and not isinstance(opt, P2PShardedAdamW)
    assert eng.zero and not eng.zero_p2p and eng.dp_p2p is None and not eng.embed_gather
    assert eng.buckets.transport == "rccl" and eng.buckets.scatter_parts is None and eng.buckets.peer is None
    n = eng.flat.numel
    S = (n // 2) // 64 * 64
    assert (opt.S, opt.lo, opt.hi, opt.n_rs, opt.n_tail) == (S, 0, S, 2 * S, n - 2 * S)
    assert eng.flat.exp_avg.numel() == S + n - 2 * S
    calls = []

    class _Prog:
        def comm(self, fn, name=None, sig=None, capturable=True):
            calls.append(sig[0][0] if sig and isinstance(sig[0], (tuple, list)) else "comm")

    opt.program = _Prog()
    refreshed = []
    monkeypatch.setattr(eng.flat, "refresh_mirror", lambda: refreshed.append(1))
    opt.step()
    assert len(calls) == (4 if opt.n_tail else 3) and refreshed == [1]
    assert eng.buckets.issued == [False] * len(eng.buckets.buckets)


# ------------------------------------------------------------------------------------------------ plan

@pytest.mark.parametrize("payload", ("fp32", "bf16"))
@pytest.mark.parametrize("W", WORLDS)
def test_zero_plan_properties(W, payload):
    e = 8 if payload == "bf16" else 4
    bks = tiled(bucket_sizes(W), start=64)
    ranges, offsets = zero_plan(bks, W, payload)
    assert len(ranges) == len(offsets) == W
    for r in range(W):
        assert len(ranges[r]) == len(bks) and len(offsets[r]) == len(bks) + 1
        cur = 0
        for i, ((a, b), (lo, hi)) in enumerate(zip(bks, ranges[r])):
            n = b - a
            pl, ph = slice_bounds(-(-n // e), W, r)
            assert (lo, hi) == (a + min(n, e * pl), a + min(n, e * ph)) == owned(a, b, W, r, payload == "bf16")
            assert a <= lo <= hi <= b and lo % 4 == 0 and hi % 4 == 0    # 16-byte aligned fp32 ranges
            assert offsets[r][i] == cur and cur % 4 == 0                  # compact offsets are contiguous
            cur += hi - lo
        assert offsets[r][-1] == cur
    for i, (a, b) in enumerate(bks):  # disjoint, in rank order, covering the bucket
        edge = a
        for r in range(W):
            lo, hi = ranges[r][i]
            if hi > lo:
                assert lo == edge
                edge = hi
        assert edge == b
    assert sum(o[-1] for o in offsets) == bks[-1][1] - bks[0][0]


@pytest.mark.parametrize("W", WORLDS)
def test_four_elements_in_bf16_leave_all_ranks_but_one_empty(W):
    ranges, offsets = zero_plan([(0, 4)], W, "bf16")
    assert ranges[0] == [(0, 4)] and all(rr[0][0] == rr[0][1] for rr in ranges[1:])
    assert [o[-1] for o in offsets] == [4] + [0] * (W - 1)


def test_zero_plan_refuses_bad_buckets():
    for bad in ([(0, 6)], [(2, 6)], [(0, 0)]):
        with pytest.raises(ValueError, match="zero plan"):
            zero_plan(bad, 2, "fp32")
    with pytest.raises(ValueError, match="payload"):
        zero_plan([(0, 8)], 2, "fp16")
    with pytest.raises(ValueError, match="ranks"):
        zero_plan([(0, 8)], 9, "fp32")


def test_half_holds_the_payload_and_the_largest_parameter_slice():
    bks = [(0, 40000), (40000, 65540)]
    assert zero_half_bytes(bks, 2, "fp32") == (160000 + 4095) // 4096 * 4096     # the fp32 payload
    assert zero_half_bytes(bks, 2, "bf16") == 81920                                # payload 80000 B == slice 20000 x 4 B
    assert zero_half_bytes(bks, 1, "bf16") == (160000 + 4095) // 4096 * 4096     # world 1: the fp32 slice is larger
    assert zero_half_bytes(bks, 1, "bf16") > dp_payload_bytes(40000, "bf16")
    assert zero_half_bytes([(0, 4)], 8, "bf16") == 4096
    for W in WORLDS:
        for payload in ("fp32", "bf16"):
            ranges, _ = zero_plan(bks, W, payload)
            half = zero_half_bytes(bks, W, payload)
            assert all(4 * (hi - lo) <= half for rr in ranges for lo, hi in rr)
            assert all(dp_payload_bytes(b - a, payload) <= half for a, b in bks)


def test_plan_hash_changes_with_world_payload_and_any_bucket_edge():
    bks = [(0, 40000), (40000, 65536), (65536, 70004)]
    h = lambda W, b, p: zero_plan_hash(W, b, p, zero_half_bytes(b, W, p))  # noqa: E731
    base = h(2, bks, "fp32")
    assert base == h(2, [tuple(b) for b in bks], "fp32")
    assert base != h(4, bks, "fp32") and base != h(2, bks, "bf16")
    assert base != h(2, [(0, 40004), (40004, 65536), (65536, 70004)], "fp32")   # an inner edge
    assert base != h(2, [(0, 40000), (40000, 65536), (65536, 70008)], "fp32")   # the last edge
    assert base != h(2, [(0, 40000), (40000, 70004)], "fp32")                   # a bucket fewer
    assert base != zero_plan_hash(2, bks, "fp32", zero_half_bytes(bks, 2, "fp32") + 4096)


def test_rs_slots():
    assert dp_rs_slots(4, "bf16", 8, 256) == 1
    assert dp_rs_slots(1100004, "fp32", 2, 256) == 256                 # capped
    assert dp_rs_slots(40004, "fp32", 2, 256) == -(-(-(-10001 // 2)) // 256)
    assert dp_rs_slots(40004, "fp32", 2, 1) == 1


# ------------------------------------------------------------------------------------------------ emulations

@pytest.mark.parametrize("W", (2, 3, 5, 8))
def test_selfcheck_emulations(W):
    n = 8 * 1031 + 4
    for bf in (False, True):
        xs = inputs(("zself", W, bf), n, W)
        full = emu_bucket(xs, bf)
        seen = torch.zeros(n, dtype=torch.bool)
        for r in range(W):
            lo, hi = owned(0, n, W, r, bf)
            got = emu_scatter(xs, r, bf)
            assert torch.equal(got[lo:hi], full[lo:hi])                    # the all-reduce's values in the slice
            assert torch.equal(got[:lo], xs[r][:lo]) and torch.equal(got[hi:], xs[r][hi:])  # nothing else moves
            assert not seen[lo:hi].any()
            seen[lo:hi] = True
        assert bool(seen.all())
        # the gather: every element from its owner, so ranks' buffers that differ everywhere give the owners' values
        ps = inputs(("zself-p", W, bf), n, W)
        g = emu_gather(ps, bf)
        for r in range(W):
            lo, hi = owned(0, n, W, r, bf)
            assert torch.equal(g[lo:hi], ps[r][lo:hi])
        assert W < 2 or not torch.equal(g, ps[0])
    m = emu_mirror(g, 100)
    assert m.dtype == BF16 and m.numel() == 100 and torch.equal(m, g[:100].to(BF16))


def test_selfcheck_sumsq_bound():
    """depth adds of products, each rounded once: relative error <= (depth + 1) u of the sum of squares (all terms
    positive), u = 2^-24; the bound grows with the depth and holds for a plain fp32 running sum."""
    assert sumsq_bound(1) < sumsq_bound(100) < sumsq_bound(10000) < 1e-2
    x = inputs(("zself-sq",), 4096, 1)[0]
    s = torch.zeros((), dtype=F32)
    for v in x:
        s = s + v * v
    ref = float((x.double() ** 2).sum())
    assert abs(float(s) - ref) <= sumsq_bound(4096) * ref
