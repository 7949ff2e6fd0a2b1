"""The embedding kernels of ``csrc/elementwise.hip`` bit for bit (docs/NUMERICS.md, "Embedding").

``embed_fwd_kernel`` adds, scales and selects; the backward (``embed_sort_kernel``, ``embed_bwd_stage1``,
``embed_segment_sum``) only adds, in an order its header calls "a pure function of the ids".  An fp32 loop on the CPU,
written from that header and from no kernel output, therefore predicts every bit of ``h``, ``dwte`` and ``dwpe``:

- keys ``id << nb | token`` (``nb = sort_bits(n)``), sorted;
- pieces of ``PIECE(n)`` sorted keys: 16 for n <= 4096, 32 for n <= 16384, else 64 (``dtc_embed_bwd``'s host constants);
- inside a piece each run of equal ids is summed sequentially in key order, from +0, into ``P[first position]``;
- ``dwte[id] = P[first key of id]``, ``+ P[b]`` for every piece boundary ``b`` inside the id's run, ascending; with
  ``beta = 1`` the old value is added last;
- ``dwpe[t]`` is the sequential sum over ``b = 0 .. B-1`` from +0, the old value last;
- the dropped gradient is ``g * sc`` with ``sc = fp32(1) / (fp32(1) - fp32(p))`` where kept and ``+0.0`` where dropped.

Independently of the order every element lies within ``c 2^-24 sum|terms|`` of the float64 sum of its ``c`` fp32 terms
(a sequential fp32 sum of c terms has at most c - 1 roundings, each at most ``2^-24`` of a partial sum that
``sum|terms|`` bounds).  The fused ``sq`` partials are held to the float64 square-sum of the kernel's own fp32 outputs:
one product, three adds and six butterfly adds per element, 10 roundings, bound ``16 2^-24`` relative (all terms
positive).  The tests whose names start with ``test_selfcheck`` need no GPU.
"""

import functools

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.ops import embedding as E

gpu = pytest.mark.gpu
U = 2.0 ** -24
GUARD = 64
F32 = np.float32


def PIECE(n):
    return 16 if n <= 4096 else (32 if n <= 16384 else 64)


# ------------------------------------------------------------------------------------------------ inputs

def _randn_wide(g, *shape):
    """randn * 10^U(-2, 2): another order or a dropped term gives other bits."""
    return (torch.randn(*shape, generator=g) * torch.pow(10.0, torch.rand(*shape, generator=g) * 4 - 2)).numpy()


def _skew_ids(g, n, V):
    """The Zipf-like ids of ``test_embedding_bwd_sorted_deterministic``: long runs of the small ids (many pieces), single
    keys of the large ones, and one run of id 7 that crosses piece boundaries."""
    r = torch.rand(n, generator=g)
    ids = torch.minimum((V ** r).long() - 1, torch.tensor(V - 1)).to(torch.int32)
    ids[: min(n, 3 * 64 + 5)] = 7
    return ids.numpy()


# name -> (B, T, D, V, kind); n = B * T
BWD_SHAPES = {
    "n1_same": (1, 1, 64, 8, "same"),
    "n3_same": (1, 3, 64, 8, "same"),
    "n64_same": (1, 64, 64, 8, "same"),
    "n4096": (8, 512, 64, 1000, "skew"),            # the last n with 16-key pieces
    "n4097": (17, 241, 64, 1000, "skew"),           # 32-key pieces, the last one holds a single key
    "n16384": (32, 512, 64, 1000, "skew"),
    "n16385": (5, 3277, 64, 1000, "skew"),          # 64-key pieces
    "n32767_edge": (1, 32767, 64, 131072, "edge"),  # largest key 0xFFFFFFFE, one 0xFFFFFFFF padding slot in the sort
    "n32768_edge": (64, 512, 64, 131072, "edge"),   # largest key 0xFFFFFFFF
    "n32768_same": (64, 512, 64, 8, "same"),        # one id over 512 pieces: 64 rounds of the 8-pieces-at-a-time walk
    "zipf": (8, 512, 64, 50304, "skew"),
    "d4": (8, 512, 4, 1000, "skew"),
    "d256": (8, 512, 256, 1000, "skew"),
    "d260": (8, 512, 260, 1000, "skew"),            # a second column block with one live lane
    "d768": (8, 512, 768, 1000, "skew"),
    "d1028": (8, 512, 1028, 1000, "skew"),
}
SEED, STEP, ROW0 = 99, 3, 2


@functools.lru_cache(maxsize=4)
def _inputs(name):
    """(ids int32 [B, T], dh fp32 [n, D], old dwte, old dwpe) of a backward case; read-only."""
    B, T, D, V, kind = BWD_SHAPES[name]
    n = B * T
    g = torch.Generator().manual_seed(sorted(BWD_SHAPES).index(name) + 1)
    if kind == "same":
        ids = np.full(n, 5, dtype=np.int32)
    elif kind == "skew":
        ids = _skew_ids(g, n, V)
    else:
        ids = torch.randint(0, V, (n,), generator=g, dtype=torch.int32).numpy()
        ids[[0, 7, n // 3]] = 0
        ids[[5, n // 2, n - 1]] = V - 1            # id V-1 on the last token: the largest key the layout can hold
    out = (ids.reshape(B, T), _randn_wide(g, n, D), _randn_wide(g, V, D), _randn_wide(g, T, D))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ emulation (CPU, fp32)

def emu_keys(ids):
    flat = ids.reshape(-1)
    nb = E.sort_bits(flat.size)
    return np.sort((flat.astype(np.uint32) << np.uint32(nb)) | np.arange(flat.size, dtype=np.uint32)), nb


def emu_scale(p):
    return F32(1) / (F32(1) - F32(p)) if p > 0 else F32(1)


def emu_dropped(dh, T, p, seed, step, row0):
    if p == 0:
        return dh
    keep = E.dropout_keep_mask(dh.shape[0], dh.shape[1], row0 * T, p, seed, step).numpy()
    return np.where(keep, dh * emu_scale(p), F32(0))


def emu_bwd(ids, g, V, old_w=None, old_p=None, reverse=False):
    """(dwte [V, D], dwpe [T, D], P [n, D] with NaN in the slots no piece sum writes, sorted keys) from the dropped
    gradient ``g``.  ``reverse`` sums each run backwards (self-check only)."""
    B, T = ids.shape
    n, D = g.shape
    keys, nb = emu_keys(ids)
    piece = PIECE(n)
    kid = (keys >> np.uint32(nb)).astype(np.int64)
    gs = g[(keys & np.uint32((1 << nb) - 1)).astype(np.int64)]
    new_id = np.ones(n, dtype=bool)
    new_id[1:] = kid[1:] != kid[:-1]
    starts = np.flatnonzero(new_id | (np.arange(n) % piece == 0))
    P = np.full((n, D), np.nan, dtype=F32)
    for s, e in zip(starts, np.append(starts[1:], n)):
        acc = np.zeros(D, dtype=F32)
        for q in (range(e - 1, s - 1, -1) if reverse else range(s, e)):
            acc = acc + gs[q]
        P[s] = acc
    dwte = np.zeros((V, D), dtype=F32) if old_w is None else old_w.copy()
    for s in np.flatnonzero(new_id):
        acc = P[s]
        b = (s // piece + 1) * piece
        while b < n and kid[b] == kid[s]:
            acc = acc + P[b]
            b += piece
        dwte[kid[s]] = acc if old_w is None else acc + old_w[kid[s]]
    acc = np.zeros((T, D), dtype=F32)
    for b in range(B):
        acc = acc + g[b * T:(b + 1) * T]
    dwpe = acc if old_p is None else acc + old_p
    return dwte, dwpe, P, keys


@functools.lru_cache(maxsize=8)
def _emu_case(name, p, beta):
    ids, dh, old_w, old_p = _inputs(name)
    B, T, D, V, _ = BWD_SHAPES[name]
    g = emu_dropped(dh, T, p, SEED, STEP, ROW0)
    return (g,) + emu_bwd(ids, g, V, old_w if beta else None, old_p if beta else None)


def emu_fwd(ids, wte, wpe, p, seed, step, row0):
    B, T = ids.shape
    h = (wte[ids.reshape(-1)] + np.tile(wpe[:T], (B, 1))).astype(F32)
    if p > 0:
        keep = E.dropout_keep_mask(B * T, wte.shape[1], row0 * T, p, seed, step).numpy()
        h = np.where(keep, h * emu_scale(p), F32(0))
    return h


# ------------------------------------------------------------------------------------------------ comparisons

def same_bits(got, exp):
    """Equal as bit patterns: -0.0 is not +0.0 and a NaN left from the fill never compares equal to a number."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    return got.shape == exp.shape and bool(np.array_equal(got.view(np.int32), exp.view(np.int32)))


def sum_bound_ratio(got_w, got_p, ids, g, old_w=None, old_p=None):
    """Worst |got - float64 sum| / (c 2^-24 sum|terms|) over dwte and dwpe; rows no id touches must be +0.0 (or the
    old value) exactly.  Returns inf on a violation of the latter."""
    B, T = ids.shape
    V, D = got_w.shape
    flat = ids.reshape(-1).astype(np.int64)
    g64 = g.astype(np.float64)
    ref, mag = np.zeros((V, D)), np.zeros((V, D))
    np.add.at(ref, flat, g64)
    np.add.at(mag, flat, np.abs(g64))
    cnt = np.bincount(flat, minlength=V).astype(np.float64)
    touched = cnt > 0
    base = np.zeros((V, D), dtype=F32) if old_w is None else old_w
    if not same_bits(got_w[~touched], base[~touched]):
        return float("inf")
    if old_w is not None:
        ref, mag, cnt = ref + old_w, mag + np.abs(old_w), cnt + 1
    err = np.abs(got_w.astype(np.float64) - ref)[touched]
    bound = (cnt[:, None] * U * mag)[touched]
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    refp, magp, c = g64.reshape(B, T, D).sum(0), np.abs(g64).reshape(B, T, D).sum(0), float(B)
    if old_p is not None:
        refp, magp, c = refp + old_p, magp + np.abs(old_p), c + 1
    errp = np.abs(got_p.astype(np.float64) - refp)
    return max(worst, float(np.max(np.where(errp == 0, 0.0, errp / np.maximum(c * U * magp, 1e-300)))))


def sq_ratio(sq, dwte, dwpe, keys, nb):
    """Worst |slot - float64 square-sum| / (16 2^-24 square-sum) over the ``sq`` partials, taken against the given fp32
    tables; inf if a slot that must be exactly +0.0 is not, or if the slot count is wrong."""
    n, (T, D) = keys.size, dwpe.shape
    dblk, nwpe = (D // 4 + 63) // 64, (T * (D // 4) + 63) // 64
    if sq.size != n * dblk + nwpe:
        return float("inf")
    kid = (keys >> np.uint32(nb)).astype(np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = kid[1:] != kid[:-1]
    rows = np.zeros((n, dblk * 256))
    rows[:, :D] = dwte[kid].astype(np.float64) ** 2
    ref_w = np.where(first[:, None], rows.reshape(n, dblk, 256).sum(-1), 0.0)
    flat = np.zeros(nwpe * 256)
    flat[:T * D] = dwpe.reshape(-1).astype(np.float64) ** 2
    ref = np.concatenate([ref_w.reshape(-1), flat.reshape(nwpe, 256).sum(-1)])
    if not same_bits(sq[ref == 0], np.zeros(int((ref == 0).sum()), dtype=F32)):
        return float("inf")
    err = np.abs(sq.astype(np.float64) - ref)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(16 * U * ref, 1e-300))))
    total = float((dwte.astype(np.float64) ** 2).sum() + (dwpe.astype(np.float64) ** 2).sum())
    return max(worst, abs(float(sq.astype(np.float64).sum()) - total) / (16 * U * total))


# ------------------------------------------------------------------------------------------------ GPU plumbing

def _guarded(rows, D, fill, dev):
    buf = torch.full((rows * D + 2 * GUARD,), 768.0, device=dev)
    view = buf[GUARD:GUARD + rows * D].view(rows, D)
    if isinstance(fill, np.ndarray):
        view.copy_(torch.tensor(fill))
    else:
        view.fill_(fill)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == 768.0).all()) and bool((buf[-GUARD:] == 768.0).all())


def _dev(a, dev):
    return torch.tensor(a).to(dev)             # a copy: the cached inputs are read-only


def _step(step, dev):
    return torch.tensor([step], dtype=torch.int64, device=dev)


def _gpu_bwd(dev, ids, dh, V, p, seed, step, row0, old_w=None, old_p=None, **kw):
    """Runs ``E.embed_bwd`` from NaN-filled tables (beta = 0) or from the old values (beta = 1)."""
    T, D = ids.shape[1], dh.shape[1]
    wbuf, dwte = _guarded(V, D, float("nan") if old_w is None else old_w, dev)
    pbuf, dwpe = _guarded(T, D, float("nan") if old_p is None else old_p, dev)
    E.embed_bwd(_dev(ids, dev), _dev(dh, dev), dwte, dwpe, p, seed, _step(step, dev), row0,
                0.0 if old_w is None else 1.0, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(wbuf) and _guards_intact(pbuf)
    return dwte.cpu().numpy(), dwpe.cpu().numpy()


# ------------------------------------------------------------------------------------------------ backward

BWD_CASES = [(name, p, 0) for name in BWD_SHAPES for p in (0.0, 0.1)] + [("n4097", 0.0, 1), ("d260", 0.1, 1)]


@gpu
@pytest.mark.parametrize("name,p,beta", BWD_CASES, ids=[f"{c[0]}-p{c[1]}-beta{c[2]}" for c in BWD_CASES])
def test_bwd_is_the_documented_sum_bit_for_bit(cuda, name, p, beta):
    ids, dh, old_w, old_p = _inputs(name)
    B, T, D, V, _ = BWD_SHAPES[name]
    g, exp_w, exp_p, _, keys = _emu_case(name, p, beta)
    dev_keys = E.embed_sort_keys(_dev(ids, cuda), V).cpu().numpy()
    assert np.array_equal(dev_keys, E.embed_sort_keys_host(ids)) and np.array_equal(dev_keys.view(np.uint32), keys)
    if name.endswith("_edge"):
        assert int(keys[0]) == 0 and int(keys[-1]) == 0xFFFFFFFF - (B * T == 32767)
    got_w, got_p = _gpu_bwd(cuda, ids, dh, V, p, SEED, STEP, ROW0, old_w if beta else None, old_p if beta else None)
    ratio = sum_bound_ratio(got_w, got_p, ids, g, old_w if beta else None, old_p if beta else None)
    nw, npe = int((got_w.view(np.int32) != exp_w.view(np.int32)).sum()), int((got_p.view(np.int32) !=
                                                                                exp_p.view(np.int32)).sum())
    print(f"embed_bwd {name} p={p} beta={beta}: err/bound {ratio:.3f}, differing bits dwte {nw} dwpe {npe}")
    assert ratio <= 1.0
    assert same_bits(got_w, exp_w) and same_bits(got_p, exp_p)


@gpu
def test_bwd_refusals(cuda):
    ids = torch.zeros(64, 512, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError):
        E.embed_sort_keys(ids, 131073)                      # id 131072 << 15 does not fit 32 bits
    dwte, dwpe = torch.full((131073, 4), 768.0, device=cuda), torch.full((512, 4), 768.0, device=cuda)
    with pytest.raises(RuntimeError):
        E.embed_bwd(ids, torch.ones(32768, 4, device=cuda), dwte, dwpe, 0.0, 0, _step(0, cuda), 0)
    assert E.embed_sort_keys(ids, 131072).numel() == 32768  # the largest legal vocab is accepted
    ids = torch.zeros(2, 4, dtype=torch.int32, device=cuda)
    w6, p6 = torch.full((8, 6), 768.0, device=cuda), torch.full((4, 6), 768.0, device=cuda)
    with pytest.raises(RuntimeError):
        E.embed_bwd(ids, torch.ones(8, 6, device=cuda), w6, p6, 0.0, 0, _step(0, cuda), 0)
    with pytest.raises(RuntimeError):
        E.embed_fwd(ids, w6, p6, 0.0, 0, _step(0, cuda), 0)
    w, pe, dh = torch.full((8, 64), 768.0, device=cuda), torch.full((4, 64), 768.0, device=cuda), torch.ones(8, 64, device=cuda)
    sq = torch.full((E.embed_sq_slots(2, 4, 64),), 768.0, device=cuda)
    prev = torch.full((8,), 768, dtype=torch.int32, device=cuda)
    with pytest.raises((AssertionError, RuntimeError)):
        E.embed_bwd(ids, dh, w, pe, 0.0, 0, _step(0, cuda), 0, 1.0, sq=sq)
    with pytest.raises((AssertionError, RuntimeError)):
        E.embed_bwd(ids, dh, w, pe, 0.0, 0, _step(0, cuda), 0, 1.0, prev_keys=prev)
    torch.cuda.synchronize()
    for t in (dwte, dwpe, w6, p6, w, pe, sq, prev):
        assert bool((t == 768).all())


# ------------------------------------------------------------------------------------------------ fused norm partials

@gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["n4096", "d260", "d768"])
def test_sq_partials_per_slot(cuda, name, p):
    ids, dh, _, _ = _inputs(name)
    B, T, D, V, _ = BWD_SHAPES[name]
    _, exp_w, exp_p, _, keys = _emu_case(name, p, 0)
    sq = torch.full((E.embed_sq_slots(B, T, D),), float("nan"), device=cuda)
    got_w, got_p = _gpu_bwd(cuda, ids, dh, V, p, SEED, STEP, ROW0, sq=sq)
    assert same_bits(got_w, exp_w) and same_bits(got_p, exp_p)      # the tables do not change with sq
    ratio = sq_ratio(sq.cpu().numpy(), got_w, got_p, keys, E.sort_bits(B * T))
    print(f"embed_bwd sq {name} p={p}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ sparse zeroing

@functools.lru_cache(maxsize=None)
def _sparse_ids():
    """A, B, C int32 [4, 64] over V = 1000.  B reuses half of A's ids, adds new ones and holds one heavy run; C is
    disjoint from B and overlaps A (rows that were zeroed after call 1 are written again in call 3)."""
    g = torch.Generator().manual_seed(11)
    A = torch.randint(0, 400, (256,), generator=g).numpy()
    ua = np.unique(A)
    reuse, rest = ua[::2], ua[1::2]
    Bv = np.concatenate([reuse[torch.randint(0, reuse.size, (128,), generator=g).numpy()],
                         torch.randint(400, 700, (88,), generator=g).numpy(), np.full(40, reuse[3])])
    Bv = Bv[torch.randperm(256, generator=g).numpy()]
    Cv = np.concatenate([rest[torch.randint(0, rest.size, (128,), generator=g).numpy()],
                         torch.randint(700, 1000, (128,), generator=g).numpy()])
    Cv = Cv[torch.randperm(256, generator=g).numpy()]
    sa, sb, sc = set(A.tolist()), set(Bv.tolist()), set(Cv.tolist())
    assert len(sa & sb) >= 20 and len(sa - sb) >= 20 and len(sb - sa) >= 20 and not (sb & sc) and len(sc & sa) >= 20
    assert int((Bv == reuse[3]).sum()) >= 40                          # crosses 16-key pieces
    return tuple(x.astype(np.int32).reshape(4, 64) for x in (A, Bv, Cv))


@functools.lru_cache(maxsize=None)
def _sparse_emu(D, p=0.1):
    out = []
    for i, ids in enumerate(_sparse_ids()):
        dh = _randn_wide(torch.Generator().manual_seed(40 + i), 256, D)
        g = emu_dropped(dh, 64, p, SEED, STEP + i, ROW0)
        out.append((ids, dh, g) + emu_bwd(ids, g, 1000))
    return out


@gpu
@pytest.mark.parametrize("D", [64, 320])
def test_sparse_zeroing_over_three_calls(cuda, D):
    V, p = 1000, 0.1
    wbuf, dwte = _guarded(V, D, float("nan"), cuda)
    prev = torch.zeros(256, dtype=torch.int32, device=cuda)
    for call, (ids, dh, g, exp_w, exp_p, _, keys) in enumerate(_sparse_emu(D)):
        dwpe = torch.full((64, D), float("nan"), device=cuda)
        sq = torch.full((E.embed_sq_slots(4, 64, D),), float("nan"), device=cuda) if call == 1 else None
        E.embed_bwd(_dev(ids, cuda), _dev(dh, cuda), dwte, dwpe, p, SEED, _step(STEP + call, cuda), ROW0, 0.0,
                    sq=sq, prev_keys=prev, prev_valid=call > 0)
        torch.cuda.synchronize()
        got_w, got_p = dwte.cpu().numpy(), dwpe.cpu().numpy()
        assert same_bits(got_w, exp_w), f"call {call + 1}: dwte is not the table of this call's ids alone"
        assert same_bits(got_p, exp_p) and _guards_intact(wbuf)
        assert np.array_equal(prev.cpu().numpy().view(np.uint32), keys), f"call {call + 1}: prev_keys"
        assert sum_bound_ratio(got_w, got_p, ids, g) <= 1.0           # includes: rows of no id are +0.0 again
        if sq is not None:
            ratio = sq_ratio(sq.cpu().numpy(), got_w, got_p, keys, E.sort_bits(256))
            print(f"embed_bwd sparse sq D={D}: worst err/bound {ratio:.3f}")
            assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ forward

def _fwd_inputs(B, T, D, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B * T,), generator=g, dtype=torch.int32).numpy()
    ids[0] = V - 1
    ids[-1] = 0 if B * T > 1 else V - 1
    return ids.reshape(B, T), _randn_wide(g, V, D), _randn_wide(g, T, D)


def _fwd_bitwise(dev, ids, wte, wpe, p, seed, step, row0):
    (B, T), D = ids.shape, wte.shape[1]
    exp = emu_fwd(ids, wte, wpe, p, seed, step, row0)
    h = E.embed_fwd(_dev(ids, dev), _dev(wte, dev), _dev(wpe, dev), p, seed, _step(step, dev), row0)
    got = h.cpu().numpy()
    assert got.shape == exp.shape and same_bits(got, exp), (int((got.view(np.int32) != exp.view(np.int32)).sum()), p)
    return got


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("D", [4, 64, 1024, 1028, 1280])
def test_fwd_bit_for_bit(cuda, D, p):
    for B, T in ((1, 1), (3, 1), (1, 5), (4, 64)):
        ids, wte, wpe = _fwd_inputs(B, T, D, 37, 1000 * D + B * T)
        assert ids.min() == 0 or B * T == 1
        assert ids.max() == 36
        got = _fwd_bitwise(cuda, ids, wte, wpe, p, 1234, 7, 3)
        if p > 0 and got.size >= 1024:
            assert abs(float((got == 0).mean()) - p) < 0.05


def _fwd_and_bwd_bitwise(dev, B, T, D, V, p, seed, step, row0):
    ids, wte, wpe = _fwd_inputs(B, T, D, V, 5)
    ids = np.arange(B * T, dtype=np.int32).reshape(B, T) % V          # every token its own row of dwte where V allows
    h = _fwd_bitwise(dev, ids, wte, wpe, p, seed, step, row0)
    dh = _randn_wide(torch.Generator().manual_seed(6), B * T, D)
    g = emu_dropped(dh, T, p, seed, step, row0)
    exp_w, exp_p, _, _ = emu_bwd(ids, g, V)
    got_w, got_p = _gpu_bwd(dev, ids, dh, V, p, seed, step, row0)
    assert same_bits(got_w, exp_w) and same_bits(got_p, exp_p)
    return h, got_w, got_p, ids


@gpu
def test_threshold_element_is_dropped_forward_and_backward(cuda):
    """Seed 1234, step 7, counter group 16500423, lane 2 draws u = 429496729: at or above ``int(0.1 * 2^32)`` and
    below the kernel's ``int(float32(0.1) * 2^32) = 429496736``.  The constants were found by a CPU search over the
    counter with ``E.philox4x32``.  With row0 = 257819, T = 4, D = 64 that draw is token 0, channel 30."""
    assert int(E.philox4x32(16500423, 0, 0, 0, 1234, 7)[2]) == 429496729
    h, dwte, dwpe, ids = _fwd_and_bwd_bitwise(cuda, 1, 4, 64, 16, 0.1, 1234, 7, 257819)
    unscaled = emu_fwd(ids, *_fwd_inputs(1, 4, 64, 16, 5)[1:], 0.0, 0, 0, 0)
    assert unscaled[0, 30] != 0 and h[0, 30].view(np.int32) == 0
    assert dwte[ids[0, 0], 30].view(np.int32) == 0 and dwpe[0, 30].view(np.int32) == 0      # B = 1, the id is unique


@gpu
def test_high_counter_word(cuda):
    """row0 = 2^26 - 1, T = 4, D = 64: the Philox group index of the first element is 2^32 - 64, so the 64-bit counter's
    high word turns 1 inside the tensor (``test_selfcheck_high_word_changes_the_mask``: dropping it changes the mask)."""
    _fwd_and_bwd_bitwise(cuda, 3, 4, 64, 16, 0.1, 1234, 7, 2 ** 26 - 1)


@gpu
def test_step_above_int32(cuda):
    _fwd_and_bwd_bitwise(cuda, 3, 4, 64, 16, 0.1, 1234, 2 ** 31 + 5, 3)


# ------------------------------------------------------------------------------------------------ CPU self-checks

def test_selfcheck_reverse_run_order_gives_other_bits():
    ids, _, _, _ = _inputs("n4096")
    g, exp_w, exp_p, _, _ = _emu_case("n4096", 0.1, 0)
    rev_w, rev_p, _, _ = emu_bwd(ids, g, 1000, reverse=True)
    assert same_bits(rev_p, exp_p) and not same_bits(rev_w, exp_w)
    rows = int((rev_w.view(np.int32) != exp_w.view(np.int32)).any(1).sum())
    assert rows >= 20, rows                                           # every id with a run of three or more, mostly
    assert sum_bound_ratio(rev_w, rev_p, ids, g) <= 1.0               # ... yet inside the order-free bound
    assert sum_bound_ratio(exp_w, exp_p, ids, g) <= 1.0
    assert PIECE(4096) == 16 and PIECE(4097) == 32 and PIECE(16384) == 32 and PIECE(16385) == 64


def test_selfcheck_high_word_changes_the_mask():
    full = E.dropout_keep_mask(12, 64, (2 ** 26 - 1) * 4, 0.1, 1234, 7).numpy()
    groups = np.arange(2 ** 32 - 64, 2 ** 32 + 128, dtype=np.uint64)
    lo = np.stack(E.philox4x32(groups & np.uint64(0xFFFFFFFF), 0, 0, 0, 1234, 7), axis=1).reshape(12, 64)
    low_only = lo >= np.uint64(E.drop_threshold(0.1))
    assert np.array_equal(full[:4], low_only[:4]) and not np.array_equal(full[4:], low_only[4:])
    assert not np.array_equal(E.dropout_keep_mask(12, 64, 12, 0.1, 1234, 2 ** 31 + 5).numpy(),
                              E.dropout_keep_mask(12, 64, 12, 0.1, 1234, 5).numpy())


def test_selfcheck_table_comparison_rejects_a_stale_row():
    (ids_a, _, _, w_a, *_), (ids_b, _, g_b, w_b, p_b, *_), _ = _sparse_emu(64)
    stale = sorted(set(ids_a.reshape(-1).tolist()) - set(ids_b.reshape(-1).tolist()))[0]
    assert same_bits(w_b[stale], np.zeros(64, dtype=F32)) and np.abs(w_a[stale]).max() > 0
    bad = w_b.copy()
    bad[stale] = w_a[stale]
    assert same_bits(w_b.copy(), w_b) and not same_bits(bad, w_b)
    assert sum_bound_ratio(bad, p_b, ids_b, g_b) == float("inf") and sum_bound_ratio(w_b, p_b, ids_b, g_b) <= 1.0
    neg = w_b.copy()
    neg[stale, 0] = -0.0
    assert not same_bits(neg, w_b)


def test_selfcheck_sq_check_rejects_piece_sums_and_a_missing_block():
    _, w, pe, P, keys = _emu_case("d260", 0.1, 0)
    n, nb, D, T = 4096, 12, 260, 512
    kid = (keys >> np.uint32(nb)).astype(np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = kid[1:] != kid[:-1]

    def partials(rows):                                               # [n, D] fp32 -> slots, summed in float64
        pad = np.zeros((n, 512))
        pad[:, :D] = rows.astype(np.float64) ** 2
        w_slots = np.where(first[:, None], pad.reshape(n, 2, 256).sum(-1), 0.0)
        p_slots = (pe.reshape(-1).astype(np.float64) ** 2).reshape(-1, 256).sum(-1)
        return np.concatenate([w_slots.reshape(-1), p_slots]).astype(F32)

    good = partials(w[kid])
    assert good.size == n * 2 + T * 65 // 64 and sq_ratio(good, w, pe, keys, nb) <= 1.0
    from_pieces = partials(np.where(first[:, None], np.nan_to_num(P), 0).astype(F32))   # P[s]: before the pieces are added
    assert sq_ratio(from_pieces, w, pe, keys, nb) > 1.0
    no_last = good.copy()
    no_last[1:2 * n:2] = 0.0                                          # the column block of channels 256 .. 259
    assert sq_ratio(no_last, w, pe, keys, nb) > 1.0
    assert sq_ratio(good[:-1], w, pe, keys, nb) == float("inf")
    off = good.copy()
    off[0] *= F32(1 + 32 * U)
    assert sq_ratio(off, w, pe, keys, nb) > 1.0
