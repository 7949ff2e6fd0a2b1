"""``pp_comm: p2p`` without a GPU: the slot-reuse proof over every supported schedule, the slot table both ends of a
message derive, and the configurations the engine refuses.

The in-graph transport keeps one slot per (sender, receiver, tag), rewritten every step.  ``check_slot_reuse``
replays two consecutive steps of all stages under the transport's semantics (sends never block; a receive completes
once the matching send has been issued) and demands a message path from the read of a slot's old content to its
next write.  The hand-written programs below show that it can fail.
"""

import itertools

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.parallel.p2p import FLAG_WORDS, pp_slot_table, pp_table_hash
from distributed_training_compare_jax_amd.parallel.pp import check_slot_reuse, graph_cuts, pp_program, simulate

BF16, F32 = torch.bfloat16, torch.float32
N = 4 * 64 * 64  # a [rows * T, D] message of the tiny model


def _accepts_head_split(kind, S):
    """What Engine.__init__ accepts: pp >= 2 and the 1f1b or zb schedule."""
    return S >= 2 and kind in ("1f1b", "zb")


# ------------------------------------------------------------------------------------------------ slot reuse

@pytest.mark.parametrize("kind", ["gpipe", "1f1b", "zb"])
@pytest.mark.parametrize("S", [2, 3, 4, 8])
def test_slot_reuse_is_ordered_for_every_schedule(kind, S):
    for M in range(1, 17):
        for hs in ((False, True) if _accepts_head_split(kind, S) else (False,)):
            c = check_slot_reuse(kind, S, M, head_split=hs)
            # every message of both steps was written and read once; every slot was reused once (step 2)
            per_step = 2 * (S - 1) * M + (2 * M if hs else 0)
            assert c == {"writes": 2 * per_step, "reads": 2 * per_step, "reuses": per_step}, (kind, S, M, hs, c)


def test_slot_reuse_three_steps():
    assert check_slot_reuse("1f1b", 4, 8, head_split=True, steps=3)["reuses"] == 2 * (2 * 3 * 8 + 16)


def _post(name, peer, snd=(), rcv=()):
    return ("post", name, peer, tuple(snd), tuple(rcv))


def test_slot_reuse_detects_a_double_send():
    """Stage 0 sends f(0) twice with no message from stage 1 in between: the second write may land before (or
    while) stage 1 reads the first content."""
    f0 = ("f", 0)
    p0 = [("F", 0), _post("a", +1, snd=[f0]), ("F", 0), _post("b", +1, snd=[f0])]
    p1 = [_post("ra", -1, rcv=[f0]), ("wait", ("ra",)), ("F", 0), _post("rb", -1, rcv=[f0]), ("wait", ("rb",)), ("F", 0)]
    with pytest.raises(RuntimeError, match="slot reuse hazard"):
        check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=1)


def test_slot_reuse_detects_a_missing_answer_across_steps():
    """A forward-only pipeline: nothing tells stage 0 that stage 1 has read step n's f(0) before step n + 1
    rewrites it.  One step alone is fine; with an answering b(0) message two steps are, too."""
    f0, b0 = ("f", 0), ("b", 0)
    p0 = [("F", 0), _post("sf", +1, snd=[f0])]
    p1 = [_post("rf", -1, rcv=[f0]), ("wait", ("rf",)), ("F", 0)]
    check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=1)
    with pytest.raises(RuntimeError, match="slot reuse hazard"):
        check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=2)
    q0 = p0 + [_post("rb", +1, rcv=[b0]), ("wait", ("rb",)), ("B", 0)]
    q1 = p1 + [("B", 0), _post("sb", -1, snd=[b0])]
    assert check_slot_reuse("hand", 2, 1, progs=[q0, q1], steps=2)["reuses"] == 2


def test_slot_reuse_detects_a_write_dated_before_the_answer():
    """The answer arrives between the producing compute item and the post: a producer that writes the slot
    directly would have run before it.  The write is dated at the compute item, so this is refused."""
    f0, b0 = ("f", 0), ("b", 0)
    p0 = [_post("rb", +1, rcv=[b0]), ("F", 0), ("wait", ("rb",)), _post("sf", +1, snd=[f0])]
    p1 = [("B", 0), _post("sb", -1, snd=[b0]), _post("rf", -1, rcv=[f0]), ("wait", ("rf",)), ("F", 0)]
    check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=1)
    with pytest.raises(RuntimeError, match="slot reuse hazard"):
        check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=2)


def test_slot_reuse_reports_a_deadlock():
    f0, b0 = ("f", 0), ("b", 0)
    p0 = [_post("rb", +1, rcv=[b0]), ("wait", ("rb",)), ("F", 0), _post("sf", +1, snd=[f0])]
    p1 = [_post("rf", -1, rcv=[f0]), ("wait", ("rf",)), ("B", 0), _post("sb", -1, snd=[b0])]
    with pytest.raises(RuntimeError, match="deadlock"):
        check_slot_reuse("hand", 2, 1, progs=[p0, p1], steps=1)


def test_graph_cuts_count_the_comm_runs():
    """One cut per run of post / wait items; stage 0 of gpipe at S = 2, M = 2: sf0, sf1 + rb1, wait + rb0, wait, ..."""
    for kind, S, M in itertools.product(("gpipe", "1f1b", "zb"), (2, 4, 8), (1, 4, 8)):
        for s in range(S):
            prog = pp_program(kind, S, s, M)
            runs = len([1 for a, b in zip([("F", 0)] + prog, prog) if b[0] in ("post", "wait") and
                        a[0] not in ("post", "wait")])
            assert graph_cuts(kind, S, s, M) == runs > 0
    assert simulate("1f1b", 8, 8)["posts"] > 0  # (the programs counted above are the ones simulate proves)


# ------------------------------------------------------------------------------------------------ slot table

def _msgs(bf=True, head_split=False):
    m = {"f": (N, BF16 if bf else F32), "b": (N, BF16 if bf else F32)}
    if head_split:
        m["fh"] = (N, BF16)
        m["s"] = (4 * 64 * 3, F32)
    return m


@pytest.mark.parametrize("S,M,hs,bf", [(2, 1, False, True), (2, 2, True, False), (3, 5, False, False),
                                       (4, 4, True, True), (8, 16, True, True), (8, 8, False, False)])
def test_slot_table_agrees_on_both_ends(S, M, hs, bf):
    t = pp_slot_table(S, M, hs, _msgs(bf, hs))
    assert len(t) == S
    n_msgs = 0
    for s in range(S):
        # both ends of every message: same offset, size, flag word, sender buffer size and dtype
        for (kind, i), e in t[s]["send"].items():
            r = t[s + e.peer]["recv"][(kind, i)]
            assert r.peer == -e.peer and tuple(r)[1:] == tuple(e)[1:], (s, kind, i, e, r)
            assert e.buf_bytes == t[s]["bytes"]
            n_msgs += 1
        # this stage's outgoing slots do not overlap and lie inside its buffer, 16-byte aligned
        spans = sorted((e.offset, e.offset + e.nbytes) for e in t[s]["send"].values())
        assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])), (s, spans)
        assert all(lo % 16 == 0 and hi <= t[s]["bytes"] for lo, hi in spans)
        # its incoming flag words are unique and dense
        flags = sorted(e.flag for e in t[s]["recv"].values())
        assert flags == list(range(t[s]["flags"])) and t[s]["flags"] <= FLAG_WORDS
        assert len(t[s]["recv"]) == sum(1 for q in range(S) for e in t[q]["send"].values() if q + e.peer == s)
    assert n_msgs == 2 * (S - 1) * M + (2 * M if hs else 0)
    if hs:  # the f message of the last pair is the compute-dtype LayerNorm output, the statistics are fp32
        assert t[S - 2]["send"][("f", 0)].dtype == "bfloat16" and t[S - 2]["send"][("s", 0)].nbytes == 4 * 64 * 3 * 4
        assert t[S - 1]["send"][("s", 0)].peer == -1 and t[S - 2]["recv"][("s", 0)].peer == +1
    # deterministic: the hash every rank exchanges at init depends on every input
    h = pp_table_hash(S, M, hs, t)
    assert h == pp_table_hash(S, M, hs, pp_slot_table(S, M, hs, _msgs(bf, hs)))
    assert h != pp_table_hash(S, M + 1, hs, pp_slot_table(S, M + 1, hs, _msgs(bf, hs)))
    assert h != pp_table_hash(S, M, hs, pp_slot_table(S, M, hs, _msgs(not bf, hs)))


def test_slot_table_refuses_what_does_not_fit():
    with pytest.raises(ValueError, match="multiple of 16"):
        pp_slot_table(2, 2, False, {"f": (6, F32), "b": (8, F32)})   # 24 bytes
    with pytest.raises(ValueError, match="multiple of 16"):
        pp_slot_table(4, 2, True, dict(_msgs(True, True), s=(7 * 3, F32)))   # 84 bytes of row statistics
    # a middle stage receives f and b of every microbatch: 2 M flag words, 1024 in the flag area
    pp_slot_table(3, FLAG_WORDS // 2, False, {"f": (4, F32), "b": (4, F32)})
    with pytest.raises(ValueError, match="flag words"):
        pp_slot_table(3, FLAG_WORDS // 2 + 1, False, {"f": (4, F32), "b": (4, F32)})
    # stage S - 2 of a split head receives f, b and s: 3 M
    with pytest.raises(ValueError, match="flag words"):
        pp_slot_table(3, FLAG_WORDS // 3 + 1, True, {"f": (4, F32), "b": (4, F32), "fh": (8, BF16), "s": (4, F32)})
    with pytest.raises(ValueError, match="no shape"):
        pp_slot_table(2, 1, True, {"f": (4, F32), "b": (4, F32)})


# ------------------------------------------------------------------------------------------------ schema / engine

def _tc(**kw):
    return TrainConfig(seed=0, parallel=kw.pop("parallel", "pp"), batch=4, steps=1, log_every=1000,
                       output_dir="/tmp/unused", **kw)


def test_pp_comm_defaults_to_rccl():
    assert _tc().pp_comm == "rccl"
    assert TrainConfig.__dataclass_fields__["pp_comm"].default == "rccl"


def _engine(tc, world, device):
    from distributed_training_compare_jax_amd.train.engine import Engine

    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=4)
    return Engine(mc, tc, OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, world, 0, torch.device(device), "gloo"))


def test_engine_rejects_unknown_pp_comm():
    for bad in ("auto", "nccl", ""):
        with pytest.raises(ValueError, match="pp_comm"):
            _engine(_tc(parallel="dp", pp_comm=bad, device="cpu"), 1, "cpu")


@pytest.mark.parametrize("what,tc_kw,world,device", [
    ("pp == 1", dict(parallel="dp"), 1, "cpu"),
    ("CPU device", dict(pp_microbatches=2), 2, "cpu"),
    ("pp=16", dict(pp_microbatches=4), 16, "cuda"),
    ("tp=2", dict(pp_microbatches=2, pp=2, tp=2), 4, "cuda"),
])
def test_engine_refuses_unsupported_p2p_layouts(what, tc_kw, world, device):
    """Raised before the engine touches the device or the process group (none exists here)."""
    with pytest.raises(ValueError, match="pp_comm: p2p cannot be combined with .*" + what):
        _engine(_tc(pp_comm="p2p", **tc_kw), world, device)
