"""Document-masked causal attention on the GPU (csrc/attention.hip doc kernels, csrc/elementwise.hip
dtc_doc_bounds): query q of row b sees key k iff doc_start[b, q] <= k <= q.

The bounds kernel is held bit for bit to a numpy loop of the definition.  The attention kernels are held to a
float64 masked softmax built from the definition, at the metrics and bounds docs/NUMERICS.md fixes for the 32-row
family (o per 16-row block 2e-2, dQ / dK / dV 3e-2, lse 1e-3 absolute), on explicit document starts that hit every
edge of the 32-row waves, the 64-key tiles and the 128-row blocks; then bit for bit: a document's rows do not
depend on any other document, a single document is the unmasked kernel of the same family, eager equals hipGraph
replays, two runs are equal, and nothing is written outside the outputs.
"""

import functools

import numpy as np
import pytest
import torch

from test_kernels_scale_gpu import BLOCK, _close_blocks, _worst_block
from test_kernels_gpu import _r

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.ops.gemm import _workspace

pytestmark = pytest.mark.gpu

SEP = 7


# ------------------------------------------------------------------------------------------------ bounds

def bounds_np(ids, sep):
    """The definition, one position at a time."""
    ids = np.asarray(ids)
    rows, T = ids.shape
    ds, de = np.zeros((rows, T), np.int32), np.zeros((rows, T), np.int32)
    for b in range(rows):
        starts = [t for t in range(T) if t == 0 or ids[b, t - 1] == sep]
        for t in range(T):
            ds[b, t] = max(s for s in starts if s <= t)
            later = [s for s in starts if s > t]
            de[b, t] = min(later) if later else T
    return ds, de


def _placements(T):
    """One row per separator placement; every other token is an ordinary id."""
    g = np.random.default_rng(T)
    base = lambda: g.integers(SEP + 1, 50, T).astype(np.int32)  # noqa: E731
    rows = {}
    rows["none"] = base()
    for name, pos in (("at0", [0]), ("at_last", [T - 1]), ("two_in_a_row", [T // 2, T // 2 + 1]), ("every", range(T)),
                      ("chunk_straddle", [254, 255, 256, 257, 511, 512, 1023, 1024, 2047, 2048]),
                      ("chunk_last_only", [255, 767]), ("chunk_first_only", [256, 1024])):
        r = base()
        for p in pos:
            if 0 <= p < T:
                r[p] = SEP
        rows[name] = r
    r = base()
    r[g.random(T) < 0.05] = SEP
    rows["random"] = r
    return rows


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200, 1024, 2049])
def test_doc_bounds_kernel(cuda, T):
    rows = _placements(T)
    ids = np.stack(list(rows.values()))
    want_s, want_e = bounds_np(ids, SEP)
    n, G_ = ids.size, 1024
    buf = torch.full((2 * n + 3 * G_,), -12345, dtype=torch.int32, device=cuda)
    ds, de = buf[G_:G_ + n].view(ids.shape), buf[2 * G_ + n:2 * G_ + 2 * n].view(ids.shape)
    ids_d = torch.from_numpy(ids).to(cuda)
    N.check(N.lib().dtc_doc_bounds(ids_d.data_ptr(), ds.data_ptr(), de.data_ptr(), ids.shape[0], T, SEP,
                                   N.stream_ptr(cuda)), "dtc_doc_bounds")
    for i, name in enumerate(rows):
        assert torch.equal(ds[i].cpu(), torch.from_numpy(want_s[i])), f"doc_start, row '{name}'"
        assert torch.equal(de[i].cpu(), torch.from_numpy(want_e[i])), f"doc_end, row '{name}'"
    for g0 in (0, G_ + n, 2 * G_ + 2 * n):
        assert bool((buf[g0:g0 + G_] == -12345).all()), f"guard words at {g0} were written"
    # the op: same arrays, and the CPU branch agrees
    s2, e2 = A.doc_bounds(ids_d, SEP)
    assert torch.equal(s2, ds) and torch.equal(e2, de)
    s3, e3 = A.doc_bounds(ids_d.cpu(), SEP)
    assert torch.equal(s3, ds.cpu()) and torch.equal(e3, de.cpu()) and s3.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ cases

STARTS = {777: [0, 1, 31, 32, 33, 64, 127, 128, 129, 300, 512, 640, 776], 200: [0, 63, 64, 65, 96, 199],
          1024: [0, 128, 256, 257, 896]}
SHAPES = [(2, 200, 2, 64), (1, 777, 2, 64), (1, 1024, 2, 64), (1, 200, 2, 128), (1, 777, 2, 128)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
FWD_K = {64: ("attn_fwd32_doc_kernel<64>",), 128: ("attn_fwd32_doc_kernel<128>",)}
BWD_K = {64: ("attn_delta_kernel<64>", "attn_bwd_merged32_doc_kernel<64>"),
         128: ("attn_delta_kernel<128>", "attn_bwd_dkdv32_doc_kernel<128>", "attn_bwd_dq32_doc_kernel<128>")}


def bounds_from_starts(rows, T):
    """doc_start / doc_end int32 [B, T] from one sorted start list per row (each begins with 0)."""
    ds, de = torch.zeros(len(rows), T, dtype=torch.int32), torch.zeros(len(rows), T, dtype=torch.int32)
    for b, starts in enumerate(rows):
        assert starts[0] == 0 and starts == sorted(set(starts)) and starts[-1] < T
        for s, e in zip(starts, starts[1:] + [T]):
            ds[b, s:e], de[b, s:e] = s, e
    return ds, de


def row_starts(B, T):
    """The explicit list in row 0; in batch-2 shapes the second row is a single document."""
    return [STARTS[T]] + [[0]] * (B - 1)


@functools.lru_cache(maxsize=None)
def case(B, T, H, hd):
    """Inputs, bounds and the float64 reference of one shape: computed once, shared, never modified."""
    qkv = _r(B, T, 3 * H * hd, seed=20, dev="cpu")
    do = _r(B, T, H * hd, seed=21, dev="cpu")
    ds, de = bounds_from_starts(row_starts(B, T), T)
    q, k, v = (t.clone().requires_grad_(True) for t in qkv.double().view(B, T, 3, H, hd).unbind(2))
    pos = torch.arange(T)
    mask = (pos[None, None, :] >= ds.long()[:, :, None]) & (pos[None, None, :] <= pos[None, :, None])  # [B, q, k]
    s = torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5
    s = s.masked_fill(~mask[:, None], float("-inf"))
    o = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), v)
    o.backward(do.double().view(B, T, H, hd))
    ref = {"o": o.detach(), "lse": torch.logsumexp(s, -1).detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    return qkv, do, ds, de, ref


def run(qkv, do, doc, H):
    o, lse = A.attn_fwd(qkv, H, doc=doc)
    fwd = A.last_launch()
    dqkv = A.attn_bwd(qkv, o, lse, do, H, doc=doc)
    return o, lse, dqkv, fwd, A.last_launch()


def on(dev, *ts):
    return tuple(t.to(dev) for t in ts)


# ------------------------------------------------------------------------------------------------ float64

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_float64(cuda, shape):
    B, T, H, hd = shape
    qkv, do, ds, de, ref = case(*shape)
    qkv_d, do_d, ds_d, de_d = on(cuda, qkv, do, ds, de)
    o, lse, dqkv, fwd, bwd = run(qkv_d, do_d, (ds_d, de_d), H)
    assert (fwd.direction, fwd.path, fwd.kernels) == ("fwd", "fwd_rows32_doc", FWD_K[hd]), fwd
    assert (bwd.direction, bwd.kernels) == ("bwd", BWD_K[hd]), bwd
    assert bwd.path == ("bwd_rows32_doc_merged" if hd == 64 else "bwd_rows32_doc_128")
    assert A.plan_fwd(B, T, H, hd, doc=True) == fwd and A.plan_bwd(B, T, H, hd, doc=True) == bwd
    nqb = -(-T // 128)
    assert fwd.launches[0].grid == B * H * nqb and bwd.launches[-1].grid == B * H * nqb * (2 if hd == 64 else 1)
    d = dqkv.view(B, T, 3, H, hd)
    outs = {"o": o.view(B, T, H, hd), "dq": d[:, :, 0], "dk": d[:, :, 1], "dv": d[:, :, 2]}
    lse_err = (lse.cpu().double() - ref["lse"]).abs().max().item()
    print(f"DOC | {shape} | lse max abs err {lse_err:.3e}")
    for n, t in outs.items():
        worst, idx = _worst_block(t, ref[n])
        print(f"DOC | {shape} | {n} | worst 16-row block {worst:.3e} at {idx}")
    assert lse_err <= 1e-3, f"lse: max abs err {lse_err:.3e} > 1e-3"
    for n, t in outs.items():
        _close_blocks(t, ref[n], 2e-2 if n == "o" else 3e-2, BLOCK, 1, n)


# ------------------------------------------------------------------------------------------------ bit for bit

@pytest.mark.parametrize("shape,doc_i", [((2, 200, 2, 64), 3), ((1, 777, 2, 64), 9), ((1, 777, 2, 64), 5),
                                         ((1, 1024, 2, 64), 1), ((1, 1024, 2, 64), 3), ((1, 200, 2, 128), 3),
                                         ((1, 777, 2, 128), 9), ((1, 777, 2, 128), 6)])
def test_documents_are_isolated(cuda, shape, doc_i):
    """q / k / v / dO of one middle document re-randomised: every other document's o, lse, dQ, dK, dV keep their
    bits.  Masked scores are replaced before the max and P is zeroed by select, so a failure is a leak."""
    B, T, H, hd = shape
    qkv, do, ds, de, _ = case(*shape)
    starts = STARTS[T]
    s, e = starts[doc_i], starts[doc_i + 1]
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[0, s:e] = _r(e - s, 3 * H * hd, seed=77, dev="cpu", scale=1.5)
    do2[0, s:e] = _r(e - s, H * hd, seed=78, dev="cpu", scale=1.5)
    doc = on(cuda, ds, de)
    a = run(*on(cuda, qkv, do), doc, H)[:3]
    b = run(*on(cuda, qkv2, do2), doc, H)[:3]
    keep = torch.ones(B, T, dtype=torch.bool, device=cuda)
    keep[0, s:e] = False
    for name, x, y in zip(("o", "lse", "dqkv"), a, b):
        if name == "lse":  # [B, H, T]
            x, y = x.transpose(1, 2), y.transpose(1, 2)
        assert torch.equal(x[keep], y[keep]), f"{name}: rows outside document [{s}, {e}) changed"
        assert not torch.equal(x[~keep], y[~keep]), f"{name}: the document's own rows did not change"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_single_document_is_the_unmasked_kernel(cuda, shape):
    """doc_start = 0, doc_end = T: the selects change no value and the arithmetic is the shared body's."""
    B, T, H, hd = shape
    qkv, do = on(cuda, *case(*shape)[:2])
    doc = (torch.zeros(B, T, dtype=torch.int32, device=cuda), torch.full((B, T), T, dtype=torch.int32, device=cuda))
    o, lse, dqkv, _, _ = run(qkv, do, doc, H)
    o0, lse0 = A.attn_fwd(qkv, H, flags=A.FwdFlags.ROUND4 if hd == 64 else 0)
    assert A.last_launch().kernels == (f"attn_fwd32_kernel<{hd}>",)
    dqkv0 = A.attn_bwd(qkv, o0, lse0, do, H, flags=A.BwdFlags.FORCE_MERGED if hd == 64 else 0)
    assert A.last_launch().path == ("bwd_rows32_merged" if hd == 64 else "bwd_rows32_128")
    assert torch.equal(o, o0) and torch.equal(lse, lse0) and torch.equal(dqkv, dqkv0)


@pytest.mark.parametrize("shape", [(2, 200, 2, 64), (1, 777, 2, 128)], ids=["2x200x2x64", "1x777x2x128"])
def test_guards_graph_and_determinism(cuda, shape):
    """o, lse and dqkv carved out of one buffer with guard words around each: the guards keep their value; two
    eager runs and three hipGraph replays give the same bits."""
    B, T, H, hd = shape
    qkv, do, ds, de = on(cuda, *case(*shape)[:4])
    L, G_ = N.lib(), 4096
    sizes = [B * T * H * hd, 2 * B * H * T, B * T * 3 * H * hd]  # o, lse (fp32 = 2 bf16 words each), dqkv: in bf16 words
    offs = [G_, 2 * G_ + sizes[0], 3 * G_ + sizes[0] + sizes[1]]
    buf = torch.empty(4 * G_ + sum(sizes), dtype=torch.bfloat16, device=cuda)
    o = buf[offs[0]:offs[0] + sizes[0]].view(B, T, H * hd)
    lse = buf[offs[1]:offs[1] + sizes[1]].view(torch.float32).view(B, H, T)
    dqkv = buf[offs[2]:offs[2] + sizes[2]].view(B, T, 3 * H * hd)
    ws = _workspace(cuda, int(L.dtc_attn_bwd_workspace_bytes(B, T, H, hd)))

    def step():
        st = N.stream_ptr(cuda)
        N.check(L.dtc_attn_fwd_doc(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, T, H, hd, 0, hd ** -0.5,
                                   ds.data_ptr(), de.data_ptr(), st), "dtc_attn_fwd_doc")
        N.check(L.dtc_attn_bwd_doc(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dqkv.data_ptr(), 0, B,
                                   T, H, hd, hd ** -0.5, ws.data_ptr(), ws.numel() * ws.element_size(), ds.data_ptr(),
                                   de.data_ptr(), st), "dtc_attn_bwd_doc")

    def fresh():
        buf.fill_(-7.25)

    fresh()
    step()
    first = buf.view(torch.int16).clone()  # bits: half an fp32 lse word read as bf16 may be a NaN pattern
    guards = [(0, G_)] + [(offs[i] + sizes[i], offs[i] + sizes[i] + G_) for i in range(3)]
    for a, b in guards:
        assert bool((buf[a:b] == -7.25).all()), f"guard words [{a}, {b}) were written"
    ref = run(qkv, do, (ds, de), H)[:3]  # the ops give what the entry points gave
    assert torch.equal(o, ref[0]) and torch.equal(lse, ref[1]) and torch.equal(dqkv, ref[2])
    fresh()
    step()
    assert torch.equal(buf.view(torch.int16), first), "two eager runs differ"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="thread_local")
        step()
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    for i in range(3):
        fresh()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int16), first), f"graph replay {i} differs from the eager run"


@pytest.mark.parametrize("hd", [32, 96])
def test_other_head_dims_are_refused(cuda, hd):
    B, T, H = 1, 64, 2
    qkv, do = _r(B, T, 3 * H * hd, seed=1), _r(B, T, H * hd, seed=2)
    doc = (torch.zeros(B, T, dtype=torch.int32, device=cuda), torch.full((B, T), T, dtype=torch.int32, device=cuda))
    A.attn_fwd(_r(1, 64, 3 * 2 * 64, seed=3), 2)  # something to leave in the record
    before = A.last_launch()
    with pytest.raises(RuntimeError, match="4005"):
        A.attn_fwd(qkv, H, doc=doc)
    with pytest.raises(RuntimeError, match="4005"):
        A.attn_bwd(qkv, torch.zeros_like(do), torch.zeros(B, H, T, device=cuda), do, H, doc=doc)
    with pytest.raises(RuntimeError, match="4005"):
        A.plan_fwd(B, T, H, hd, doc=True)
    with pytest.raises(RuntimeError, match="4005"):
        A.plan_bwd(B, T, H, hd, doc=True)
    assert A.last_launch() == before
    with pytest.raises(NotImplementedError):
        A.attn_fwd(_r(1, 64, 3 * 2 * 64, seed=3, dtype=torch.float32), 2, doc=doc)
