"""The evaluation head's kernels on the GPU: the logits-free lm_head + CE epilogue (``EPI_LMHEAD_EVAL``,
``csrc/gemm.hip lmhead_rows<EVAL>``), the top-1 finish (``ce_eval_finish_rows``) and the exact-fp32 mode's streaming
row arg-max (``row_argmax_f32_kernel``).

The reference is the storing kernel (``EPI_LMHEAD``, ``ops.xent.lmhead_logits_partials``): the new epilogue's row
statistics and label logit must be ITS bits, and the arg-max the first maximum over the valid columns of the bf16
logits IT stores, so no rounding can move a comparison.  The tie cases use integer-valued operands whose fp32 partial
sums are all exact: the bf16-rounded logits are then known exactly from a float64 product, and ``numpy.argmax`` (first
occurrence) is the expected column of every row.

Shapes: 2048 x 50304 x 256 (``n_valid`` 50258) is the shape ``tests/test_gemm_floor_gpu.py::test_floor_lmhead_logits``
uses to reach the DMA-staged 256^2 kernel (1576 tiles, ragged last N tile, two whole 64-column parts past N);
2024 rows leave the last M tile ragged (``mvalid``); 200 x 1024 x 128 (``n_valid`` 1000) stays below the big-tile
threshold: the register-staged 128^2 kernel, ragged in M, pads inside the last part.  Every case first asserts from
``ops.gemm.last_launch()`` which family and epilogue ran."""

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.ops import _native as N

gpu = pytest.mark.gpu

BIG = dict(M=2048, D=256, V=50258, Vp=50304, fam=dict(family="gemm8p_kernel", bm=256, bn=256, sub=4, split_k=1))
BIG_RAGGED = dict(BIG, M=2048 - 24)
SMALL = dict(M=200, D=128, V=1000, Vp=1024, fam=dict(family="gemm_kernel", bm=128, bn=128, sub=64, split_k=1))
SHAPES = {"big256": BIG, "big256_ragged_m": BIG_RAGGED, "small128": SMALL}


def _ran(fam, epi, what):
    from distributed_training_compare_jax_amd.ops import gemm as G

    ll = G.last_launch()
    for k, v in dict(fam, epi=epi).items():
        assert getattr(ll, k) == v, f"{what}: expected {k}={v}, ran {ll}"


def _gauss(sh, mean):
    """bf16 h, W and fp32 b; ``mean`` shifts the activations and the bias (large-mean logits: the row statistics then
    live far from 0, where a max / sum-exp slip shows)."""
    g = torch.Generator().manual_seed(1234 + sh["M"] + int(mean))
    h = (torch.randn(sh["M"], sh["D"], generator=g) + 0.25 * mean).to(torch.bfloat16).cuda()
    w = (0.2 * torch.randn(sh["Vp"], sh["D"], generator=g)).to(torch.bfloat16).cuda()
    b = (torch.randn(sh["Vp"], generator=g) + 10.0 * mean).cuda()
    labels = torch.randint(0, sh["V"], (sh["M"],), dtype=torch.int32, generator=g).cuda()
    return h, w, b, labels


# tie placements: (first column, second column) relative to the 256-column tile `t0`; the same pairs serve the 128^2
# kernel, whose waves also hold 64 columns as 4 fragments x 4 lane groups x 4 columns (column = 16 i + 4 g + r)
def _tie_pairs(sh):
    t0 = 256
    V = sh["V"]
    return [
        ("one lane's four columns", t0 + 16 + 4, t0 + 16 + 6),
        ("two lane groups of one wave", t0 + 32 + 1, t0 + 32 + 9),
        ("two 64-column parts of one tile", t0 + 3, t0 + 64 + 7),
        ("two tiles", 9, 2 * t0 + 64 * 2 + 9),
        ("valid column and pad column", V - 1, V),  # the pad gets the LARGER value and must still lose
    ]


def _ties(sh, dtype=torch.bfloat16):
    """Integer operands: features [0, ncat) are one-hot category selectors (row m belongs to category m % ncat), the
    rest small integers; the two columns of a pair share one weight row and bias, so they tie on EVERY row, and on
    their category's rows the selector lifts them above everything else.  |logit| <= 2 S + 2 (D - ncat) << 2^24 and
    every product and partial sum is an integer: exact in fp32 in any order."""
    M, D, V, Vp = sh["M"], sh["D"], sh["V"], sh["Vp"]
    pairs = _tie_pairs(sh)
    ncat, S = len(pairs), 400
    g = torch.Generator().manual_seed(77 + M)
    h = torch.randint(-1, 2, (M, D), generator=g).float()
    w = torch.randint(-1, 2, (Vp, D), generator=g).float()
    b = torch.randint(-3, 4, (Vp,), generator=g).float()
    h[:, :ncat] = 0.0
    w[:, :ncat] = 0.0
    rows = torch.arange(M)
    h[rows, rows % ncat] = 1.0
    labels = torch.randint(0, V, (M,), dtype=torch.int32, generator=g)
    for k, (name, c1, c2) in enumerate(pairs):
        w[c2] = w[c1]
        b[c2] = b[c1]
        w[c1, k] = S
        w[c2, k] = 2 * S if c2 >= V else S
        mine = rows[rows % ncat == k]
        labels[mine[0::2]] = c1  # the label on the first tied column: correct
        if c2 < V:
            labels[mine[1::2]] = c2  # on the second: the lower column wins, so not correct
    return h.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda(), labels.cuda(), pairs


def _exact_logits(h, w, b, V):
    """The bf16-rounded logits, exactly: float64 product of the integer operands (exact), one rounding to bf16."""
    ref = h.double() @ w.double().t() + b.double()
    return ref[:, :V].to(torch.bfloat16).float()


_CACHE = {}


def _both(key, sh, h, w, b, labels):
    """(storing kernel's logits, part, lab) and (the evaluation epilogue's part, lab, cand_val, cand_col), once."""
    from distributed_training_compare_jax_amd.ops import xent as X

    if key not in _CACHE:
        logits, part, lab = X.lmhead_logits_partials(h, w, b, labels, 0, sh["V"], combine=False)
        _ran(sh["fam"], N.EPI_LMHEAD, f"{key}: storing head")
        ev = X.lmhead_eval_partials(h, w, b, labels, 0, sh["V"])
        _ran(sh["fam"], N.EPI_LMHEAD_EVAL, f"{key}: evaluation head")
        torch.cuda.synchronize()
        _CACHE.clear()  # one shape's tensors at a time (412 MB of logits at the big shape)
        _CACHE[key] = (logits, part, lab, ev)
    return _CACHE[key]


def _first_argmax(x):
    """First maximum per row of x [M, V] (torch.argmax does not promise the first one on the GPU)."""
    mx = x.max(-1, keepdim=True).values
    idx = torch.arange(x.shape[1], device=x.device, dtype=torch.int32)
    return torch.where(x == mx, idx, torch.full_like(idx, 2**31 - 1)).min(-1).values


@gpu
@pytest.mark.parametrize("mean", [0.0, 3.0], ids=["gaussian", "large_mean"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_statistics_are_the_storing_kernels(cuda, shape, mean):
    """part, label_out, then lse and loss after ce_finalize: torch.equal to the storing kernel's."""
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SHAPES[shape]
    h, w, b, labels = _gauss(sh, mean)
    logits, part, lab, (part2, lab2, cval, ccol) = _both((shape, mean), sh, h, w, b, labels)
    assert part2.shape == part.shape and ccol.shape == part.shape[:2]
    assert torch.equal(part2, part), f"{shape}: row statistics differ from EPI_LMHEAD's"
    assert torch.equal(lab2, lab), f"{shape}: label logits differ from EPI_LMHEAD's"
    lse, loss = X.ce_finalize(part, lab, 1.0 / sh["M"])
    lse2, loss2 = X.ce_finalize(part2, lab2, 1.0 / sh["M"])
    assert torch.equal(lse2, lse) and torch.equal(loss2, loss)
    assert bool(torch.isfinite(loss).all())


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_argmax_general(cuda, shape):
    """Every part's candidate is the first maximum of its 64 columns of the STORED logits (valid columns only, -1 where
    it has none), and the finished arg-max the first maximum over all valid columns, for every row."""
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SHAPES[shape]
    M, V = sh["M"], sh["V"]
    h, w, b, labels = _gauss(sh, 0.0)
    logits, part, lab, (part2, lab2, cval, ccol) = _both((shape, 0.0), sh, h, w, b, labels)
    P = ccol.shape[0]
    lg = torch.full((M, P * 64), float("-inf"), device="cuda")
    lg[:, :V] = logits[:, :V].float()
    per = lg.view(M, P, 64)
    pmax = per.max(-1).values                                    # [M, P]
    loc = _first_argmax(per.reshape(M * P, 64)).view(M, P)
    exp_col = torch.where(pmax == float("-inf"), torch.full_like(loc, -1),
                          loc + 64 * torch.arange(P, device="cuda", dtype=torch.int32)[None])
    assert torch.equal(cval.t(), pmax), f"{shape}: part maxima"
    assert torch.equal(ccol.t(), exp_col), f"{shape}: per-part arg-max"
    assert int((ccol == -1).sum()) == M * (P - (V + 63) // 64)   # exactly the parts past the last valid column
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    am, val, correct = X.ce_eval_finish(cval, ccol, 0, labels, count)
    exp = _first_argmax(lg[:, :V])
    assert torch.equal(am, exp), f"{shape}: {int((am != exp).sum())} rows differ"
    assert torch.equal(val, lg[:, :V].max(-1).values)
    assert torch.equal(correct, (exp == labels).int()) and int(count) == int((exp == labels).sum())


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_argmax_constructed_ties(cuda, shape):
    """Row maxima placed twice (within a lane's four columns, across lane groups, parts and tiles, in a valid and a
    pad column, the label on the first and on the second tied column): numpy.argmax per row, exactly, and the count."""
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SHAPES[shape]
    M, V = sh["M"], sh["V"]
    h, w, b, labels, pairs = _ties(sh)
    logits, part, lab, (part2, lab2, cval, ccol) = _both((shape, "ties"), sh, h, w, b, labels)
    ref = _exact_logits(h, w, b, V)
    assert torch.equal(logits[:, :V].float(), ref), "the integer logits are not the exact ones: the test's premise"
    ref_np = ref.cpu().numpy()
    exp = np.argmax(ref_np, axis=1).astype(np.int32)  # first occurrence
    ncat = len(pairs)
    for k, (name, c1, c2) in enumerate(pairs):  # the construction did what it says
        mine = np.arange(M)[np.arange(M) % ncat == k]
        assert (exp[mine] == c1).all(), name
        if c2 < V:
            assert (ref_np[mine, c1] == ref_np[mine, c2]).all() and (ref_np[mine].max(1) == ref_np[mine, c1]).all(), name
    assert torch.equal(part2, part) and torch.equal(lab2, lab)
    count = torch.full((1,), 5, dtype=torch.int32, device="cuda")  # ADDED to
    am, val, correct = X.ce_eval_finish(cval, ccol, 0, labels, count)
    assert np.array_equal(am.cpu().numpy(), exp), f"{shape}: rows {np.nonzero(am.cpu().numpy() != exp)[0][:8]}"
    exp_ok = exp == labels.cpu().numpy()
    assert np.array_equal(correct.cpu().numpy(), exp_ok.astype(np.int32))
    assert int(count) == 5 + int(exp_ok.sum()) and 0 < int(exp_ok.sum()) < M


@gpu
@pytest.mark.parametrize("shape", ["big256_ragged_m", "small128"])
def test_no_logits_written_and_neighbours_untouched(cuda, shape):
    """The output pointer is null, and the three outputs, carved out of one buffer with guard words between and
    around them, leave every guard word as it was."""
    from distributed_training_compare_jax_amd.ops import gemm as G
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SHAPES[shape]
    M, D, V, Vp = sh["M"], sh["D"], sh["V"], sh["Vp"]
    h, w, b, labels = _gauss(sh, 0.0)
    P = int(N.lib().dtc_lmhead_nparts(M, Vp, D))
    G_ = 4096  # guard words (16 KB) before, between and after
    sizes = [P * M * 2, M, P * M]
    buf = torch.full((G_ * 4 + sum(sizes),), -7.25, dtype=torch.float32, device="cuda")
    offs, o = [], G_
    for n in sizes:
        offs.append(o)
        o += n + G_
    part = buf[offs[0]:offs[0] + sizes[0]].view(P, M, 2)
    lab = buf[offs[1]:offs[1] + M]
    col = buf[offs[2]:offs[2] + sizes[2]].view(torch.int32).view(P, M)
    lab.zero_()
    G._gemm_native(0, M, Vp, D, h, h.stride(0), w, w.stride(0), None, Vp, epi=N.EPI_LMHEAD_EVAL, bias=b, labels=labels,
                   vocab_start=0, n_valid=V, part=part, label_out=lab, part_arg=col)
    _ran(sh["fam"], N.EPI_LMHEAD_EVAL, shape)
    torch.cuda.synchronize()
    guards = [buf[:G_]] + [buf[offs[i] + sizes[i]:offs[i] + sizes[i] + G_] for i in range(3)]
    for i, gd in enumerate(guards):
        assert bool((gd == -7.25).all()), f"guard {i} was written"
    part2, lab2, _, col2 = X.lmhead_eval_partials(h, w, b, labels, 0, V)
    assert torch.equal(part, part2) and torch.equal(lab, lab2) and torch.equal(col, col2)


@gpu
@pytest.mark.parametrize("shape", ["big256", "small128"])
def test_replay_from_a_graph(cuda, shape):
    """Captured once, replayed three times: the same bits each time, the eager ones."""
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SHAPES[shape]
    h, w, b, labels = _gauss(sh, 0.0)

    def run():
        part, lab, cval, ccol = X.lmhead_eval_partials(h, w, b, labels, 0, sh["V"])
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        am, _, correct = X.ce_eval_finish(cval, ccol, 0, labels, count)
        lse, loss = X.ce_finalize(part, lab, 1.0 / sh["M"])
        return part, lab, ccol, am, correct, count, lse, loss

    eager = [t.clone() for t in run()]
    _ran(sh["fam"], N.EPI_LMHEAD_EVAL, shape)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for i in range(3):
        for t in outs:  # every output is rewritten by the replay
            t.fill_(float("nan") if t.dtype == torch.float32 else -3)
        g.replay()
        torch.cuda.synchronize()
        for name, a, e in zip("part lab ccol argmax correct count lse loss".split(), outs, eager):
            assert torch.equal(a, e), f"{shape}: replay {i}: {name} differs from the eager run"


@gpu
@pytest.mark.parametrize("widths", [(384, 640), (256, 448, 320)], ids=["R2", "R3"])
def test_vocab_parallel_combine(cuda, widths):
    """The vocabulary split over R shards of unequal widths on one GPU, with a tie across shards: per shard the
    evaluation head and its winner, the shards' (max, sum exp, column) stacked as the TP gather stacks them, one finish
    over the fp32-held columns -- the single-shard arg-max, correct flags and count, exactly."""
    from distributed_training_compare_jax_amd.ops import gemm as G
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SMALL
    M, V = sh["M"], sh["V"]
    h, w, b, labels, pairs = _ties(sh)
    name, c1, c2 = pairs[3]
    bounds = np.cumsum((0,) + widths)
    assert bounds[-1] == sh["Vp"] and np.searchsorted(bounds, c1, "right") != np.searchsorted(bounds, c2, "right"), \
        f"'{name}' must straddle two shards"
    part, lab, cval, ccol = X.lmhead_eval_partials(h, w, b, labels, 0, V)
    count1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    am1, val1, ok1 = X.ce_eval_finish(cval, ccol, 0, labels, count1)
    packs, labsum = [], torch.zeros(M, device="cuda")
    for s, e in zip(bounds[:-1], bounds[1:]):
        s, e = int(s), int(e)
        p, l, cv, cc = X.lmhead_eval_partials(h, w[s:e], b[s:e], labels, s, max(0, min(e - s, V - s)), single_shard=False)
        assert G.last_launch().epi == N.EPI_LMHEAD_EVAL and G.last_launch().family == "gemm_kernel"
        mine, _, _ = X.ce_eval_finish(cv, cc, s)
        packs.append(torch.cat([X.combine_partials(p), mine.float()[:, None]], 1))
        labsum += l
    g = torch.stack(packs)  # [R, M, 3]
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    am, val, ok = X.ce_eval_finish(g[:, :, 0], g[:, :, 2], 0, labels, count)
    assert torch.equal(am, am1) and torch.equal(val, val1) and torch.equal(ok, ok1) and int(count) == int(count1)
    assert torch.equal(labsum, lab)


@gpu
def test_fp32_fallback_argmax(cuda):
    """dtype fp32: the storing exact-fp32 head + the streaming row arg-max over its stored logits, on the same tie
    cases (integer operands are exact in fp32 as they are); and the kernel alone at a width that is no multiple of 4,
    a tie across threads, a pad that is larger, and a row with no valid column."""
    from distributed_training_compare_jax_amd.ops import xent as X

    sh = SMALL
    M, V = sh["M"], sh["V"]
    h, w, b, labels, pairs = _ties(sh, torch.float32)
    logits, part, lab = X.lmhead_logits_partials(h, w, b, labels, 0, V, combine=False)
    part2, lab2, cval, ccol = X.lmhead_eval_partials(h, w, b, labels, 0, V)
    assert torch.equal(part2, part) and torch.equal(lab2, lab) and cval.shape == (1, M)
    ref = (h.double() @ w.double().t() + b.double())[:, :V].float()
    assert torch.equal(logits[:, :V], ref)
    exp = np.argmax(ref.cpu().numpy(), axis=1).astype(np.int32)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    am, val, ok = X.ce_eval_finish(cval, ccol, 0, labels, count)
    assert np.array_equal(am.cpu().numpy(), exp)
    assert int(count) == int((exp == labels.cpu().numpy()).sum())
    # the kernel alone
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-50, 50, (37, 2052), generator=g).float()
    nv = 2041  # 2041 = 4 * 510 + 1: a scalar tail
    x[0, 3] = x[0, 1500] = 99.0       # two threads' columns tie: the lower one
    x[1, 2040] = 99.0                 # the tail column
    x[2, 2045] = 1e9                  # a pad: never a candidate
    x[3, 0] = x[3, 1] = 99.0          # inside one float4
    x = x.cuda()
    v = torch.empty(37, device="cuda")
    a = torch.empty(37, dtype=torch.int32, device="cuda")
    N.check(N.lib().dtc_row_argmax_f32(x.data_ptr(), x.stride(0), 37, nv, v.data_ptr(), a.data_ptr(),
                                       N.stream_ptr(x.device)), "dtc_row_argmax_f32")
    xe = x[:, :nv].cpu().numpy()
    assert np.array_equal(a.cpu().numpy(), np.argmax(xe, 1).astype(np.int32))
    assert np.array_equal(v.cpu().numpy(), xe.max(1))
    assert a[0] == 3 and a[1] == 2040 and a[3] == 0
    N.check(N.lib().dtc_row_argmax_f32(x.data_ptr(), x.stride(0), 37, 0, v.data_ptr(), a.data_ptr(),
                                       N.stream_ptr(x.device)), "dtc_row_argmax_f32")
    assert bool((a == -1).all())
