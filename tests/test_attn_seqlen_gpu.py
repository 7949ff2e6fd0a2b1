"""Attention at the sequence lengths no other suite launches: T = 2048 (the length of the 1.3B presets: 16 query
blocks of 128 rows, 32 key tiles of 64) and T below one 16-row MFMA tile, one 32-row wave and one 64-key tile, on
every kernel family: head_dim 32 chunked and resident, the head_dim 64 forwards and backwards, head_dim 128, the
exact-fp32 kernels, grouped-query and document-masked attention (docs/NUMERICS.md, "Attention: sequence length").

Every case first asserts which kernels ran (``A.last_launch()`` against ``A.plan_fwd`` / ``A.plan_bwd`` and the
expected names).  The bounds are the project's own: o per 16-row block at 2e-2 of the block's maximum, dQ / dK / dV
at 3e-2, lse 1e-3 absolute, against float64 torch on the rounded inputs (no kernel output feeds a reference); the
exact-fp32 kernels at 4x the worst block of ``test_f32_floor_gpu._attn_emulate32`` on the same shape and input.
At T = 1 the references of dQ and dK are exactly zero (dS = p (dP - delta) with p = 1 and delta = dP), so they are
judged absolutely against the size of the terms that cancel (``_self_scale``).  The short cases run B = 2, H = 2: a
read past row T of batch 0 lands in batch 1's rows and shows as a wrong value.  ``test_guards_*`` carve outputs and
inputs out of sentinel-filled buffers and hold the words around them.

The unmarked tests need no GPU: they show that the bf16 emulation of a correct kernel sits at no more than half of
every bound used here, and that the metrics reject the mutants a long or a short sequence would produce.
"""

import functools

import pytest
import torch

import test_attention_hd128_gpu as HD128
import test_attn_doc_gpu as DOC
import test_attn_gqa_gpu as GQA
from test_f32_floor_gpu import MARGIN, _attn_case32, _attn_emulate32
from test_kernels_f32_gpu import _r as _r32
from test_kernels_gpu import _attn_ref64, _close, _r
from test_kernels_scale_gpu import (BLOCK, BWD_FAMILY, FWD_FAMILY, _attn_case, _attn_emulate, _attn_inputs, _bf,
                                    _block_ratios, _close_blocks, _worst_block)

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.ops.gemm import _workspace

gpu = pytest.mark.gpu
FF, BF = A.FwdFlags, A.BwdFlags
O_TOL, G_TOL, LSE_TOL = 2e-2, 3e-2, 1e-3  # docs/NUMERICS.md: o, dQ / dK / dV per 16-row block; lse absolute
F32_ULP = 2.0 ** -24  # one rounding to fp32
NAMES = ("o", "dq", "dk", "dv")

# family -> head_dim, the forwards and the backwards as (flags, kernels that must run)
MHA = {
    "chunk32": (32, [(0, FWD_FAMILY["chunk32", 0])], [(0, BWD_FAMILY["chunk32", 0])]),
    "res32": (32, [(f, FWD_FAMILY["res32", f]) for f in (0, FF.PLAIN_WAVES)],
              [(f, BWD_FAMILY["res32", f]) for f in (0, BF.TWO_ROUND)]),
    "hd64": (64, [(f, FWD_FAMILY["hd64", f]) for f in (0, FF.WPS2, FF.ROUND4, FF.CHUNK16)],
             [(f, BWD_FAMILY["hd64", f]) for f in (0, BF.FORCE_MERGED, BF.CHUNK16)]),
    "hd128": (128, [(0, HD128.FWD_KERNELS)], [(0, HD128.BWD_KERNELS)]),
}
SHORT_T = (1, 3, 15, 16, 17, 31, 33, 63)
RES_T = (4, 16, 60)  # resident head_dim 32: T % 4 == 0
# The input seed of every short T: the first even seed from 20 at which the bf16 emulation stays below a third of each
# bound in all of that T's cases (T = 3: the best of the first fifty, 0.35 of the bound;
# test_selfcheck_short_floor_is_half_the_bound asserts half).  A seed is a property
# of the input alone.  It matters here because a ragged 16-row block may hold ONE row (T = 17, 33), and dK / dV of the
# last key come from one (query, key) pair: the block's maximum is then one dS = p (dP - delta), which an unlucky draw
# makes as small as the rounding of delta (rowsum(dO * bf16 O)) -- at T = 33, seed 24 the emulation alone is 88x over.
SEEDS = {1: 20, 3: 78, 4: 24, 15: 24, 16: 24, 17: 22, 31: 26, 33: 20, 60: 20, 63: 22}
LONG_DOC_STARTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 1151, 1152, 1920, 2047]


# ------------------------------------------------------------------------------------ references and emulation

def _heads(qkv, do, H, Hkv):
    B, T, C = qkv.shape
    hd = C // (H + 2 * Hkv)
    q, k, v = qkv.double().split([H * hd, Hkv * hd, Hkv * hd], -1)
    return hd, q.view(B, T, H, hd), k.view(B, T, Hkv, hd), v.view(B, T, Hkv, hd), do.double().view(B, T, H, hd)


def _mask(T, ds, dev):
    """[B or 1, q, k]: query q sees key k iff doc_start[b, q] <= k <= q (no bounds: k <= q)."""
    pos = torch.arange(T, device=dev)
    see = (pos[None, :] <= pos[:, None])[None]
    return see if ds is None else see & (pos[None, None, :] >= ds.to(dev).long()[:, :, None])


def _ref64(qkv, do, H, Hkv=None, ds=None, dev="cpu"):
    """float64 autograd through the materialised masked softmax on the rounded inputs, one K/V head with its G query
    heads at a time (the [B, H, T, T] score tensor never exists whole), on ``dev``.  No kernel output feeds it.
    o, dq [B, T, H, hd], lse [B, H, T], dk, dv [B, T, Hkv, hd], on the CPU."""
    Hkv = Hkv or H
    G, T = H // Hkv, qkv.shape[1]
    hd, q, k, v, dof = _heads(qkv.to(dev), do.to(dev), H, Hkv)
    mask = _mask(T, ds, dev)
    parts = {n: [] for n in ("o", "lse", "dq", "dk", "dv")}
    for j in range(Hkv):
        qj, kj, vj = (t.clone().requires_grad_(True) for t in (q[:, :, j * G:(j + 1) * G], k[:, :, j], v[:, :, j]))
        s = torch.einsum("btgd,bsd->bgts", qj, kj) * hd ** -0.5
        s = s.masked_fill(~mask[:, None], float("-inf"))
        o = torch.einsum("bgts,bsd->btgd", torch.softmax(s, -1), vj)
        o.backward(dof[:, :, j * G:(j + 1) * G])
        for n, t in zip(parts, (o.detach(), torch.logsumexp(s, -1).detach(), qj.grad, kj.grad, vj.grad)):
            parts[n].append(t.cpu())
        del s, o
    return {"o": torch.cat(parts["o"], 2), "lse": torch.cat(parts["lse"], 1), "dq": torch.cat(parts["dq"], 2),
            "dk": torch.stack(parts["dk"], 2), "dv": torch.stack(parts["dv"], 2)}


def _emulate(qkv, do, H, Hkv=None, ds=None):
    """``test_kernels_scale_gpu._attn_emulate`` (P and dS rounded to bf16 before their second matmul, outputs rounded
    to bf16, everything else exact) with a document mask and grouped K/V heads: dK / dV of a K/V head are summed over
    its group before the one rounding, as the kernels sum them in fp32 registers.  Hkv = H, no bounds: that function."""
    Hkv = Hkv or H
    B, T, G = qkv.shape[0], qkv.shape[1], H // Hkv
    hd, q, k, v, dof = _heads(qkv, do, H, Hkv)
    k, v = (t.repeat_interleave(G, 2) for t in (k, v))
    s = torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5
    s = s.masked_fill(~_mask(T, ds, "cpu")[:, None], float("-inf"))
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    o = _bf(torch.einsum("bhts,bshd->bthd", _bf(p), v))
    delta = (dof * o).sum(-1).permute(0, 2, 1)
    dsc = p * (torch.einsum("bthd,bshd->bhts", dof, v) - delta[..., None]) * hd ** -0.5
    dv = torch.einsum("bhts,bthd->bshd", _bf(p), dof)
    dq = _bf(torch.einsum("bhts,bshd->bthd", _bf(dsc), k))
    dk = torch.einsum("bhts,bthd->bshd", _bf(dsc), q)
    dk, dv = (_bf(t.view(B, T, Hkv, G, hd).sum(3)) for t in (dk, dv))
    return {"o": o, "dq": dq, "dk": dk, "dv": dv}


def _self_scale(qkv, do, H, Hkv=None):
    """A row that sees only itself (T = 1; a document of one row): p = 1 and delta = dP, so dS = 0 and the references
    of its dQ and dK are exactly zero; a relative bound has no scale there.  What a kernel leaves is the rounding of
    the two sums that cancel, dP = sum_d dO_d v_d and delta, times hd^-1/2 and k (dQ) or q (dK; summed over the group
    of a K/V head).  The size of those terms, from the inputs alone: hd^-1/2 sum_d |dO_d v_d| max|k| per row
    [B, T, H, 1] and, with max|q|, [B, T, Hkv, 1].  bf16 is held to 3e-2 of it, the relative bound of every other
    block; fp32 to 2 hd 2^-24 of it (_run_f32)."""
    Hkv = Hkv or H
    B, T, G = qkv.shape[0], qkv.shape[1], H // Hkv
    hd, q, k, v, dof = _heads(qkv, do, H, Hkv)
    k, v = (t.repeat_interleave(G, 2) for t in (k, v))
    terms = hd ** -0.5 * (dof * v).abs().sum(-1)  # [B, T, H]
    return {"dq": (terms * k.abs().amax(-1))[..., None],
            "dk": (terms * q.abs().amax(-1)).view(B, T, Hkv, G).sum(-1)[..., None]}


def _figure(name, out, ref, zs=None):
    """(relative, absolute): the worst 16-row block's max|out - ref| / max|ref| over the blocks whose reference is not
    exactly zero, and over those where it is (dQ / dK of rows that see only themselves) the worst max|out - ref| in
    units of the block's ``_self_scale``."""
    err, mag = _block_ratios(out, ref, BLOCK, 1)
    zero = mag == 0
    rel = (err / mag.clamp_min(1e-300))[~zero].max().item() if bool((~zero).any()) else 0.0
    if not bool(zero.any()):
        return rel, 0.0
    assert zs is not None and name in zs, f"{name}: a block of the reference is exactly zero"
    scale = _block_ratios(zs[name], zs[name], BLOCK, 1)[1]
    return rel, (err / scale)[zero].max().item()


def _hold(family, shape, outs, ref, floor, bounds, zs=None, abs_bound=G_TOL):
    """Prints every SEQLEN line, then asserts every tensor: ``_close_blocks`` at ``bounds[name]``; where the reference
    has exactly-zero blocks, those at ``abs_bound`` of their cancelling terms and the others at ``bounds[name]``."""
    figs = {n: _figure(n, t, ref[n], zs) for n, t in outs.items()}
    for n, (rel, ab) in figs.items():
        fl = floor[n] if isinstance(floor[n], tuple) else (floor[n], 0.0)
        print(f"SEQLEN | {family} | {n} | {shape} | kernel {rel:.3e} | emulation {fl[0]:.3e} | "
              f"ratio {rel / fl[0] if fl[0] else float('nan'):.2f} | bound {bounds[n]:.3e}"
              + (f" | zero-reference blocks: kernel {ab:.3e} of the cancelling terms | emulation {fl[1]:.3e} | "
                 f"bound {abs_bound:.3e}" if ab or fl[1] else ""))
    for n, t in outs.items():
        rel, ab = figs[n]
        if bool((_block_ratios(t, ref[n], BLOCK, 1)[1] == 0).any()):
            assert rel <= bounds[n], f"{n}: worst 16-row block {rel:.3e} > {bounds[n]:.3e}"
            assert ab <= abs_bound, f"{n}: {ab:.3e} of the cancelling terms > {abs_bound:.3e}"
        else:
            _close_blocks(t, ref[n], bounds[n], BLOCK, 1, n)


def _hold_lse(family, shape, lse, ref, bound=LSE_TOL, floor=float("nan")):
    err = (lse.cpu().double() - ref["lse"]).abs().max().item()
    print(f"SEQLEN | {family} | lse | {shape} | kernel {err:.3e} abs | emulation {floor:.3e} | bound {bound:.3e}")
    assert err <= bound, f"lse: max abs err {err:.3e} > {bound:.3e}"


BF16_BOUNDS = {"o": O_TOL, "dq": G_TOL, "dk": G_TOL, "dv": G_TOL}


def _short_starts(B, T):
    """Row 0: documents of one row at both ends ([0, 1, T - 1], T >= 3); every other row a single document."""
    return [[0, 1, T - 1] if T >= 3 else [0]] + [[0]] * (B - 1)


@functools.lru_cache(maxsize=None)
def _case(B, T, H, Hkv, hd, doc=False, seed=20):
    """bf16 inputs (Hkv = H, seed 20: those of ``_attn_inputs``), bounds, float64 reference and the bf16 emulation's
    figures of one short shape: computed once on the CPU, shared, never modified."""
    qkv, do = _r(B, T, (H + 2 * Hkv) * hd, seed=seed, dev="cpu"), _r(B, T, H * hd, seed=seed + 1, dev="cpu")
    ds, de = DOC.bounds_from_starts(_short_starts(B, T), T) if doc else (None, None)
    ref = _ref64(qkv, do, H, Hkv, ds)
    zs = _self_scale(qkv, do, H, Hkv)
    emu = _emulate(qkv, do, H, Hkv, ds)
    return qkv, do, ds, de, ref, {n: _figure(n, emu[n], ref[n], zs) for n in NAMES}, zs


def _long(B, T, H, hd, spike=False):
    """``_attn_case`` of test_kernels_scale_gpu (cached there): inputs, float64 reference, emulation floors."""
    return _attn_case(B, T, H, hd, spike)


# ------------------------------------------------------------------------------------------------ running

def _run(cuda, shape, H, hd, fwds, bwds, case, family, tensors=("dq", "dk", "dv"), Hkv=None, doc=None, zs=None,
         hold_fwd=True):
    """Every forward of ``fwds`` and, on the first one's o and lse (as in training), every backward of ``bwds``: the
    record equals the plan and names the expected kernels, then the bounds."""
    B, T = shape[0], shape[1]
    qkv, do, ref, floor = case
    qkv_d, do_d = qkv.to(cuda), do.to(cuda)
    kw, pkw = {}, {}
    if Hkv:
        kw, pkw = dict(n_kv_heads=Hkv), dict(n_kv_heads=Hkv)
    if doc is not None:
        kw, pkw = dict(doc=tuple(t.to(cuda) for t in doc)), dict(doc=True)
    first = None
    for flags, kernels in fwds:
        o, lse = A.attn_fwd(qkv_d, H, flags=flags, **kw)
        rec = A.last_launch()
        assert rec == A.plan_fwd(B, T, H, hd, flags, **pkw) and (rec.direction, rec.kernels) == ("fwd", kernels), rec
        first = first or (o, lse)
        label = f"{family} {' + '.join(kernels)}" + (f", flags {int(flags)}" if flags else "")
        if hold_fwd:
            _hold_lse(label, shape, lse, ref)
            _hold(label, shape, {"o": o.view(B, T, H, hd)}, ref, floor, BF16_BOUNDS)
    for flags, kernels in bwds:
        dqkv = A.attn_bwd(qkv_d, first[0], first[1], do_d, H, flags=flags, **kw)
        rec = A.last_launch()
        assert rec == A.plan_bwd(B, T, H, hd, flags, **pkw) and (rec.direction, rec.kernels) == ("bwd", kernels), rec
        dq, dk, dv = dqkv.split([H * hd, (Hkv or H) * hd, (Hkv or H) * hd], -1)
        outs = {"dq": dq.view(B, T, H, hd), "dk": dk.view(B, T, -1, hd), "dv": dv.view(B, T, -1, hd)}
        label = f"{family} {' + '.join(kernels)}" + (f", flags {int(flags)}" if flags else "")
        _hold(label, shape, {n: outs[n] for n in tensors}, ref, floor, BF16_BOUNDS, zs)
    return first


def _run_f32(cuda, shape, qkv, do, ref, floor, zs=None):
    """The exact-fp32 kernels leave no record (A.last_launch is the bf16 kernels'): the record must not move."""
    B, T, H, hd = shape
    before = A.last_launch()
    qkv_d, do_d = qkv.to(cuda), do.to(cuda)
    o, lse = A.attn_fwd(qkv_d, H)
    assert o.dtype == torch.float32 and lse.shape == (B, H, T)
    d = A.attn_bwd(qkv_d, o, lse, do_d, H).view(B, T, 3, H, hd)
    assert d.dtype == torch.float32 and A.last_launch() == before
    outs = {"o": o.view(B, T, H, hd), "dq": d[:, :, 0], "dk": d[:, :, 1], "dv": d[:, :, 2]}
    bounds = {n: MARGIN * floor[n] for n in NAMES}  # T = 1: o = v and the emulation is exact; so is the kernel
    _hold_lse(f"attn_f32<{hd}>", shape, lse, ref, MARGIN * floor["lse"], floor["lse"])
    # zero-reference blocks (T = 1): two fp32 chains of hd products cancel, each within hd 2^-24 sum|dO_d v_d| of exact
    _hold(f"attn_f32<{hd}>", shape, outs, ref, floor, bounds, zs, abs_bound=2 * hd * F32_ULP)


# ------------------------------------------------------------------------------------------ 1. T = 2048

LONG = [pytest.param((1, 2048, 2, 128), "hd128", id="1x2048x2x128"),
        pytest.param((1, 2000, 2, 128), "hd128", id="1x2000x2x128"),
        pytest.param((1, 2048, 2, 64), "hd64", id="1x2048x2x64"), pytest.param((1, 2048, 2, 32), "chunk32", id="1x2048x2x32")]


@gpu
@pytest.mark.parametrize("shape,family", LONG)
def test_long_bf16(cuda, shape, family):
    """16 query blocks, 32 key tiles (T = 2000: a ragged last 128-row block and a ragged last 64-key tile), every
    forward and backward of the family against float64 per 16-row block."""
    B, T, H, hd = shape
    _, fwds, bwds = MHA[family]
    _run(cuda, shape, H, hd, fwds, bwds, _long(B, T, H, hd), family)


@functools.lru_cache(maxsize=None)
def _case32_long(B, T, H, hd, dev):
    """As test_f32_floor_gpu._attn_case32 builds it (same inputs, reference and emulation), with the emulation's
    float64 / fp32 torch arithmetic placed on ``dev``: its 2 T sequential steps take minutes on the CPU at T = 2048."""
    qkv, do = _r32(B, T, 3 * H * hd, seed=16), _r32(B, T, H * hd, seed=17)
    o, lse, dqkv = _attn_ref64(qkv, do, H)
    dq, dk, dv = dqkv.view(B, T, 3, H, hd).unbind(2)
    ref = {"o": o.view(B, T, H, hd), "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    with torch.device(dev):
        emu, emu_lse = _attn_emulate32(qkv.to(dev), do.to(dev), H)
    floor = {n: _worst_block(emu[n], ref[n])[0] for n in emu}
    floor["lse"] = (emu_lse.cpu().double() - lse).abs().max().item()
    return qkv, do, ref, floor


@gpu
@pytest.mark.parametrize("shape", [(1, 2048, 2, 128), (1, 2000, 2, 128)], ids=["1x2048x2x128", "1x2000x2x128"])
def test_long_f32(cuda, shape):
    _run_f32(cuda, shape, *_case32_long(*shape, str(cuda)))


SPIKE = (1, 2048, 2, 128)
# Decided on the CPU (test_selfcheck_spike_dq_decision holds this constant to the computation): at this shape the
# float64 emulation of the bf16 rounding of O alone -- delta = rowsum(dO * bf16(O)), every other step exact -- leaves
# more than 3e-2 of a block's maximum in dQ, so no backward on a bf16 O can meet the bound: a strict xfail, as
# test_kernels_scale_gpu.SPIKE_DQ at T = 1024.
SPIKE_DQ_OVER = True
SPIKE_DQ = pytest.mark.xfail(strict=True, reason="delta = rowsum(dO * O) from the bf16-rounded O: over 3e-2 per block in "
                             "the float64 emulation of that rounding alone (docs/NUMERICS.md)")


def _dq_o_rounding_alone(qkv, do, H):
    """dQ in float64 with one step inexact: delta from the bf16-rounded O."""
    B, T, _ = qkv.shape
    hd, q, k, v, dof = _heads(qkv, do, H, H)
    s = torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5
    s = s.masked_fill(~_mask(T, None, "cpu")[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    delta = (dof * _bf(torch.einsum("bhts,bshd->bthd", p, v))).sum(-1).permute(0, 2, 1)
    dsc = p * (torch.einsum("bthd,bshd->bhts", dof, v) - delta[..., None]) * hd ** -0.5
    return torch.einsum("bhts,bshd->bthd", dsc, k)


@gpu
@pytest.mark.parametrize("tensors", [pytest.param(("dk", "dv"), id="o-lse-dk-dv"),
                                     pytest.param(("dq",), id="dq", marks=[SPIKE_DQ] if SPIKE_DQ_OVER else [])])
def test_long_spike(cuda, tensors):
    """One key mid-sequence scaled 12x (``_attn_inputs(..., spike=True)``): o, lse, dK and dV are asserted; dQ as
    SPIKE_DQ_OVER decides, in a case of its own that asserts nothing else."""
    B, T, H, hd = SPIKE
    _, fwds, bwds = MHA["hd128"]
    _run(cuda, SPIKE, H, hd, fwds, bwds, _long(B, T, H, hd, True), "hd128 spike", tensors, hold_fwd="dk" in tensors)


@gpu
@pytest.mark.parametrize("H,Hkv,hd", [(16, 4, 128), (4, 1, 64)])
def test_long_gqa(cuda, H, Hkv, hd):
    """The GQA preset's own head layout (gqa_block's transposed order at H = 16, G = 4) and the merged head_dim 64
    kernel at T = 2048: o, lse, dQ bit for bit against the 32-row multi-head kernels on repeated K/V heads; dK / dV
    against float64, one K/V head at a time, dO of each group's first query head scaled 16x (test_attn_gqa_gpu)."""
    B, T, G = 1, 2048, H // Hkv
    w = [H * hd, Hkv * hd, Hkv * hd]
    qkv, do = _r(B, T, sum(w), seed=30), _r(B, T, H, hd, seed=31)
    do[:, :, ::G] *= 16
    do = do.view(B, T, H * hd)
    o, lse = A.attn_fwd(qkv, H, n_kv_heads=Hkv)
    fwd = A.last_launch()
    dqkv = A.attn_bwd(qkv, o, lse, do, H, n_kv_heads=Hkv)
    bwd = A.last_launch()
    assert fwd == A.plan_fwd(B, T, H, hd, n_kv_heads=Hkv) and bwd == A.plan_bwd(B, T, H, hd, n_kv_heads=Hkv)
    assert (fwd.path, fwd.kernels, fwd.launches[0].grid) == ("fwd_rows32_gqa", (f"attn_fwd32_gqa_kernel<{hd}>",), B * H * 16)
    assert (bwd.path, bwd.kernels) == GQA.BWD[hd], bwd
    q, k, v = qkv.split(w, -1)
    kr, vr = (t.view(B, T, Hkv, hd).repeat_interleave(G, 2).view(B, T, H * hd) for t in (k, v))
    rep = torch.cat([q, kr, vr], -1).contiguous()
    o0, lse0 = A.attn_fwd(rep, H, flags=FF.ROUND4 if hd == 64 else 0)
    assert A.last_launch().kernels == (f"attn_fwd32_kernel<{hd}>",)
    d0 = A.attn_bwd(rep, o0, lse0, do, H, flags=BF.FORCE_MERGED if hd == 64 else 0)
    assert A.last_launch().path == ("bwd_rows32_merged" if hd == 64 else "bwd_rows32_128")
    assert torch.equal(o, o0) and torch.equal(lse, lse0) and torch.equal(dqkv[..., :H * hd], d0[..., :H * hd])
    ref = _ref64(qkv, do, H, Hkv, dev=cuda)
    for n, t in zip(("dk", "dv"), dqkv.split(w, -1)[1:]):
        worst, idx = _worst_block(t.view(B, T, Hkv, hd), ref[n])
        print(f"SEQLEN | gqa {' + '.join(bwd.kernels)} | {n} | {(B, T, H, Hkv, hd)} | kernel {worst:.3e} at {idx}")
    for n, t in zip(("dk", "dv"), dqkv.split(w, -1)[1:]):
        _close_blocks(t.view(B, T, Hkv, hd), ref[n], G_TOL, BLOCK, 1, n)


@functools.lru_cache(maxsize=None)
def _doc_long(hd, dev):
    B, T, H = 1, 2048, 2
    qkv, do = _r(B, T, 3 * H * hd, seed=20, dev="cpu"), _r(B, T, H * hd, seed=21, dev="cpu")
    ds, de = DOC.bounds_from_starts([LONG_DOC_STARTS], T)
    return qkv, do, ds, de, _ref64(qkv, do, H, H, ds, dev=dev)


@gpu
@pytest.mark.parametrize("hd", [64, 128])
def test_long_doc(cuda, hd):
    """A packed row that is long: documents of one row at both ends, starts on both sides of the 64-key, 128-row and
    1024 boundaries, one document of 768 rows over six query blocks; against the float64 masked softmax."""
    B, T, H = 1, 2048, 2
    qkv, do, ds, de, ref = _doc_long(hd, str(cuda))
    qkv_d, do_d, doc = qkv.to(cuda), do.to(cuda), (ds.to(cuda), de.to(cuda))
    o, lse, dqkv, fwd, bwd = DOC.run(qkv_d, do_d, doc, H)
    assert fwd == A.plan_fwd(B, T, H, hd, doc=True) and bwd == A.plan_bwd(B, T, H, hd, doc=True)
    assert (fwd.path, fwd.kernels, bwd.kernels) == ("fwd_rows32_doc", DOC.FWD_K[hd], DOC.BWD_K[hd]), (fwd, bwd)
    d = dqkv.view(B, T, 3, H, hd)
    outs = {"o": o.view(B, T, H, hd), "dq": d[:, :, 0], "dk": d[:, :, 1], "dv": d[:, :, 2]}
    _hold_lse(f"doc<{hd}>", (B, T, H, hd), lse, ref)
    _hold(f"doc<{hd}>", (B, T, H, hd), outs, ref, dict.fromkeys(NAMES, float("nan")), BF16_BOUNDS)


@gpu
@pytest.mark.parametrize("hd", [64, 128])
def test_long_doc_isolated(cuda, hd):
    """test_attn_doc_gpu.test_documents_are_isolated for the 768-row document [1152, 1920): its q / k / v / dO
    re-randomised, every other document's o, lse, dQ, dK, dV keep their bits."""
    B, T, H = 1, 2048, 2
    qkv, do, ds, de, _ = _doc_long(hd, str(cuda))
    s, e = 1152, 1920
    assert LONG_DOC_STARTS[9:11] == [s, e]
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[0, s:e] = _r(e - s, 3 * H * hd, seed=77, dev="cpu", scale=1.5)
    do2[0, s:e] = _r(e - s, H * hd, seed=78, dev="cpu", scale=1.5)
    doc = (ds.to(cuda), de.to(cuda))
    a = DOC.run(qkv.to(cuda), do.to(cuda), doc, H)[:3]
    b = DOC.run(qkv2.to(cuda), do2.to(cuda), doc, H)[:3]
    keep = torch.ones(B, T, dtype=torch.bool, device=cuda)
    keep[0, s:e] = False
    for name, x, y in zip(("o", "lse", "dqkv"), a, b):
        if name == "lse":
            x, y = x.transpose(1, 2), y.transpose(1, 2)
        assert torch.equal(x[keep], y[keep]), f"{name}: rows outside document [{s}, {e}) changed"
        assert not torch.equal(x[~keep], y[~keep]), f"{name}: the document's own rows did not change"


@gpu
def test_long_balanced_order_bitwise(cuda):
    """B H = 48 with 16 query blocks: 96 blocks per XCD, the second grid that meets fw_order_n's one-round condition
    (test_attention_fwd_balanced_order_bitwise runs B H = 96 with 8).  The record must say the balanced order was
    taken, and o and lse equal the heavy-first launch bit for bit.  The arithmetic is pinned by (1, 2048, 2, 64)."""
    B, T, H, hd = 4, 2048, 12, 64
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if not (cus % 8 == 0 and cus // 8 * 3 == 96):
        pytest.skip(f"{cus} CUs: 768 blocks are not one round of 3 blocks per CU on 8 XCDs")
    qkv = _r(B, T, 3 * H * hd, seed=44)
    o, lse = A.attn_fwd(qkv, H)
    rec = A.last_launch()
    assert rec == A.plan_fwd(B, T, H, hd)
    assert (rec.kernels, rec.order, rec.order_n) == (("attn_fwd5_kernel<64,3>",), "balanced", 96), rec
    assert rec.launches[0].grid == 768, rec
    o6, lse6 = A.attn_fwd(qkv, H, flags=FF.HEAVY_FIRST)
    rec = A.last_launch()
    assert (rec.kernels, rec.order, rec.order_n) == (("attn_fwd5_kernel<64,3>",), "heavy_first", 0), rec
    assert torch.equal(o, o6) and torch.equal(lse, lse6)


# ------------------------------------------------------------------------------------------ 2. below one tile

SHORT_MHA = ([("chunk32", T) for T in SHORT_T if T % 4] + [("res32", T) for T in RES_T]
             + [(f, T) for f in ("hd64", "hd128") for T in SHORT_T])


@gpu
@pytest.mark.parametrize("family,T", SHORT_MHA, ids=[f"{f}-T{T}" for f, T in SHORT_MHA])
def test_short_bf16(cuda, family, T):
    hd, fwds, bwds = MHA[family]
    qkv, do, _, _, ref, floor, zs = _case(2, T, 2, 2, hd, False, SEEDS[T])
    _run(cuda, (2, T, 2, hd), 2, hd, fwds, bwds, (qkv, do, ref, floor), family, zs=zs)


@gpu
@pytest.mark.parametrize("T", SHORT_T + RES_T[::2])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_short_f32(cuda, hd, T):
    qkv, do, ref, floor = _attn_case32(2, T, 2, hd)
    _run_f32(cuda, (2, T, 2, hd), qkv, do, ref, floor, _self_scale(qkv, do, 2))


@gpu
@pytest.mark.parametrize("T", SHORT_T)
@pytest.mark.parametrize("hd", [64, 128])
def test_short_gqa(cuda, hd, T):
    H, Hkv = 4, 2
    qkv, do, _, _, ref, floor, zs = _case(2, T, H, Hkv, hd, False, SEEDS[T])
    _run(cuda, (2, T, H, Hkv, hd), H, hd, [(0, (f"attn_fwd32_gqa_kernel<{hd}>",))], [(0, GQA.BWD[hd][1])],
         (qkv, do, ref, floor), "gqa", Hkv=Hkv, zs=zs)


@gpu
@pytest.mark.parametrize("T", SHORT_T)
@pytest.mark.parametrize("hd", [64, 128])
def test_short_doc(cuda, hd, T):
    qkv, do, ds, de, ref, floor, zs = _case(2, T, 2, 2, hd, True, SEEDS[T])
    _run(cuda, (2, T, 2, hd), 2, hd, [(0, DOC.FWD_K[hd])], [(0, DOC.BWD_K[hd])], (qkv, do, ref, floor), "doc",
         doc=(ds, de), zs=zs)


# ----------------------------------------------------------------------------- 3. nothing outside the outputs

GUARD = 4096  # bytes around every carved tensor
# head_dim 32 at T = 200 is resident (T % 4 == 0, T <= 512): the chunked pair gets the odd T = 203 instead
GUARD_CASES = [("chunk32", 32, 203, None, torch.bfloat16, 0, 0), ("chunk32", 32, 17, None, torch.bfloat16, 0, 0),
               ("res32", 32, 60, None, torch.bfloat16, 0, 0), ("res32", 32, 16, None, torch.bfloat16, 0, 0),
               ("hd64", 64, 200, None, torch.bfloat16, 0, 0), ("hd64", 64, 17, None, torch.bfloat16, 0, 0),
               ("hd64-chunk16", 64, 200, None, torch.bfloat16, FF.CHUNK16, BF.CHUNK16),
               ("hd64-chunk16", 64, 17, None, torch.bfloat16, FF.CHUNK16, BF.CHUNK16),
               ("hd128", 128, 200, None, torch.bfloat16, 0, 0), ("hd128", 128, 17, None, torch.bfloat16, 0, 0),
               ("gqa", 64, 200, 2, torch.bfloat16, 0, 0), ("gqa", 64, 17, 2, torch.bfloat16, 0, 0),
               ("gqa", 128, 200, 2, torch.bfloat16, 0, 0), ("gqa", 128, 17, 2, torch.bfloat16, 0, 0)] + [
    ("f32", hd, T, None, torch.float32, 0, 0) for hd in (32, 64, 128) for T in (200, 17)]
GUARD_KERNELS = {"chunk32": (FWD_FAMILY["chunk32", 0], BWD_FAMILY["chunk32", 0]),
                 "res32": (FWD_FAMILY["res32", 0], BWD_FAMILY["res32", 0]),
                 "hd64": (FWD_FAMILY["hd64", 0], BWD_FAMILY["hd64", 0]),
                 "hd64-chunk16": (FWD_FAMILY["hd64", FF.CHUNK16], BWD_FAMILY["hd64", BF.CHUNK16]),
                 "hd128": (HD128.FWD_KERNELS, HD128.BWD_KERNELS)}


def _carve(dev, nbytes, fill):
    """One uint8 buffer filled with ``fill`` holding tensors of ``nbytes`` with GUARD bytes before, between and after
    them; returns (buffer, byte offsets)."""
    offs, pos = [], GUARD
    for n in nbytes:
        assert n % 16 == 0
        offs.append(pos)
        pos += n + GUARD
    return torch.full((pos,), fill, dtype=torch.uint8, device=dev), offs


@gpu
@pytest.mark.parametrize("family,hd,T,Hkv,dtype,fflags,bflags", GUARD_CASES,
                         ids=[f"{c[0]}-hd{c[1]}-T{c[2]}" for c in GUARD_CASES])
def test_guards_and_determinism(cuda, family, hd, T, Hkv, dtype, fflags, bflags):
    """test_attn_doc_gpu.test_guards_graph_and_determinism for the other families, through the C entry points: o,
    lse and dqkv carved out of one sentinel-filled buffer, qkv and dO out of another whose margins hold huge finite
    values (a read a few rows past the end stays inside the allocation and poisons the result).  The guards keep
    their value, two runs leave the same bits, and the results are the ops' on tensors of their own."""
    B, H = 2, 4 if Hkv else 2
    hkv, es, f32 = Hkv or H, torch.empty(0, dtype=dtype).element_size(), dtype == torch.float32
    W = (H + 2 * hkv) * hd
    L, scale = N.lib(), hd ** -0.5
    src = (_r32 if f32 else functools.partial(_r, dev="cpu"))
    qkv0, do0 = src(B, T, W, seed=50).to(cuda), src(B, T, H * hd, seed=51).to(cuda)
    ibuf, ioffs = _carve(cuda, [B * T * W * es, B * T * H * hd * es], 0x7F)  # bf16 0x7F7F = 3.4e38, fp32 the same
    qkv = ibuf[ioffs[0]:ioffs[0] + qkv0.numel() * es].view(dtype).view(B, T, W)
    do = ibuf[ioffs[1]:ioffs[1] + do0.numel() * es].view(dtype).view(B, T, H * hd)
    qkv.copy_(qkv0)
    do.copy_(do0)
    sizes = [B * T * H * hd * es, B * H * T * 4, B * T * W * es]
    buf, offs = _carve(cuda, sizes, 0xA5)
    o = buf[offs[0]:offs[0] + sizes[0]].view(dtype).view(B, T, H * hd)
    lse = buf[offs[1]:offs[1] + sizes[1]].view(torch.float32).view(B, H, T)
    dqkv = buf[offs[2]:offs[2] + sizes[2]].view(dtype).view(B, T, W)
    ws = _workspace(cuda, int(L.dtc_attn_bwd_workspace_bytes(B, T, H, hd)))
    p = lambda t: t.data_ptr()  # noqa: E731

    def step():
        st = N.stream_ptr(cuda)
        if f32:
            N.check(L.dtc_attn_f32_fwd(p(qkv), p(o), p(lse), B, T, H, hd, scale, st), "f32 fwd")
            N.check(L.dtc_attn_f32_bwd(p(qkv), p(o), p(lse), p(do), p(dqkv), B, T, H, hd, scale, p(ws), ws.numel(), st),
                    "f32 bwd")
        elif Hkv:
            N.check(L.dtc_attn_fwd_gqa(p(qkv), p(o), p(lse), B, T, H, Hkv, hd, 0, scale, st), "gqa fwd")
            N.check(L.dtc_attn_bwd_gqa(p(qkv), p(o), p(lse), p(do), p(dqkv), 0, B, T, H, Hkv, hd, scale, p(ws), ws.numel(), st),
                    "gqa bwd")
        else:
            N.check(L.dtc_attn_fwd(p(qkv), p(o), p(lse), B, T, H, hd, int(fflags), scale, st), "fwd")
            fwd = A.last_launch()
            N.check(L.dtc_attn_bwd(p(qkv), p(o), p(lse), p(do), p(dqkv), int(bflags), B, T, H, hd, scale, p(ws),
                                   ws.numel(), st), "bwd")
            assert (fwd.kernels, A.last_launch().kernels) == GUARD_KERNELS[family], (fwd, A.last_launch())

    step()
    torch.cuda.synchronize()
    first = buf.clone()
    for a, b in [(0, GUARD)] + [(offs[i] + sizes[i], offs[i] + sizes[i] + GUARD) for i in range(3)]:
        assert bool((buf[a:b] == 0xA5).all()), f"guard bytes [{a}, {b}) were written"
    if Hkv:
        rec = A.last_launch()
        assert rec == A.plan_bwd(B, T, H, hd, n_kv_heads=Hkv) and rec.kernels == GQA.BWD[hd][1], rec
    kw = dict(n_kv_heads=Hkv) if Hkv else {}
    o1, lse1 = A.attn_fwd(qkv0, H, flags=fflags, **kw)
    d1 = A.attn_bwd(qkv0, o1, lse1, do0, H, flags=bflags, **kw)
    assert torch.equal(o, o1) and torch.equal(lse, lse1) and torch.equal(dqkv, d1), "carved tensors differ from the ops'"
    assert bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(o.float()).all())
    buf.fill_(0xA5)
    step()
    torch.cuda.synchronize()
    assert torch.equal(buf, first), "two runs differ"


# ------------------------------------------------------------------------------------------ 4. CPU self-checks

def _half(floor):
    for n in NAMES:
        rel, ab = floor[n] if isinstance(floor[n], tuple) else (floor[n], 0.0)
        assert rel <= 0.5 * BF16_BOUNDS[n], f"{n}: emulation {rel:.3e} > half of {BF16_BOUNDS[n]:.1e}"
        assert ab <= 0.5 * G_TOL, f"{n}: emulation {ab:.3e} of the cancelling terms > half of {G_TOL:.1e}"


@pytest.mark.parametrize("shape", [(1, 2048, 2, 128), (1, 2048, 2, 64), (1, 2000, 2, 128)],
                         ids=["1x2048x2x128", "1x2048x2x64", "1x2000x2x128"])
def test_selfcheck_long_floor_is_half_the_bound(shape):
    """The bf16 emulation -- a correct kernel's rounding and nothing else -- sits at no more than half of every bound:
    the condition under which a correct kernel alone stays within it."""
    floor = _long(*shape)[3]
    print(f"SEQLEN-FLOOR | {shape} | " + " | ".join(f"{n} {v:.3e}" for n, v in floor.items()))
    _half(floor)


@pytest.mark.parametrize("T", sorted(set(SHORT_T + RES_T)))
def test_selfcheck_short_floor_is_half_the_bound(T):
    """... at every T below one tile, every head_dim, with grouped K/V heads and with document bounds (T = 1: dQ and
    dK in units of ``_self_scale``, against the same 3e-2)."""
    cases = [(2, 2, hd, False) for hd in (32, 64, 128)]
    if T in SHORT_T:
        cases += [(4, 2, hd, False) for hd in (64, 128)] + [(2, 2, hd, True) for hd in (64, 128)]
    for H, Hkv, hd, doc in cases:
        floor = _case(2, T, H, Hkv, hd, doc, SEEDS[T])[5]
        print(f"SEQLEN-FLOOR | {(2, T, H, Hkv, hd)}{' doc' if doc else ''} | "
              + " | ".join(f"{n} {v[0]:.3e}" for n, v in floor.items()))
        _half(floor)


def test_selfcheck_emulation_extends_attn_emulate():
    """Hkv = H and no bounds: ``_emulate`` is ``_attn_emulate`` to the bit and ``_ref64`` is ``_attn_ref64`` to float64
    rounding; with document bounds ``_ref64`` is test_attn_doc_gpu's reference."""
    B, T, H, hd = 2, 33, 2, 64
    qkv, do = _attn_inputs(B, T, H, hd, False)
    mine, theirs = _emulate(qkv, do, H), _attn_emulate(qkv, do, H)
    assert all(torch.equal(mine[n], theirs[n]) for n in NAMES)
    o, lse, dqkv = _attn_ref64(qkv, do, H)
    ref = _ref64(qkv, do, H)
    same = functools.partial(torch.testing.assert_close, rtol=1e-12, atol=1e-14)  # another einsum: another sum order
    same(ref["o"].reshape(B, T, H * hd), o)
    same(ref["lse"], lse)
    same(torch.stack([ref["dq"], ref["dk"], ref["dv"]], 2).reshape(B, T, 3 * H * hd), dqkv)
    qkv, do, ds, _, want = DOC.case(2, 200, 2, 64)
    got = _ref64(qkv, do, 2, 2, ds)
    for n in want:
        same(got[n], want[n])


def test_selfcheck_long_mutants_are_rejected():
    """float64 only, (1, 2048, 2, 64).  o with the last 64-key tile dropped from every query row of the last 128-row
    block, and dK / dV with their last 16 key rows zeroed, pass the whole-tensor ``_close`` and fail per block."""
    B, T, H, hd = 1, 2048, 2, 64
    qkv, do, ref, _ = _long(B, T, H, hd)
    _, q, k, v, _ = _heads(qkv, do, H, H)
    rows = slice(T - 128, T)
    s = torch.einsum("bthd,bshd->bhts", q[:, rows], k) * hd ** -0.5
    pos = torch.arange(T)
    see = (pos[None, :] <= pos[rows, None]) & (pos[None, :] < T - 64)  # keys of the last tile dropped
    bad = ref["o"].clone()
    bad[:, rows] = torch.einsum("bhts,bshd->bthd", torch.softmax(s.masked_fill(~see, float("-inf")), -1), v)
    assert torch.equal(bad[:, :T - 64], ref["o"][:, :T - 64]) and not torch.equal(bad, ref["o"])
    _close(bad, ref["o"], O_TOL, "o, last key tile dropped (whole-tensor metric)")
    with pytest.raises(AssertionError, match="worst 16-row block"):
        _close_blocks(bad, ref["o"], O_TOL, BLOCK, 1, "o")
    for n in ("dk", "dv"):
        bad = ref[n].clone()
        bad[:, T - BLOCK:] = 0
        _close(bad, ref[n], G_TOL, f"{n}, last block zeroed (whole-tensor metric)")
        with pytest.raises(AssertionError, match="worst 16-row block"):
            _close_blocks(bad, ref[n], G_TOL, BLOCK, 1, n)
        _close_blocks(ref[n], ref[n], G_TOL, BLOCK, 1, n)


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_selfcheck_short_mutant_is_rejected(hd):
    """T = 17: a result that ignores row 16 (computed as if T = 16, padded with zeros) is rejected in every tensor."""
    qkv, do, _, _, ref, _, _ = _case(2, 17, 2, 2, hd, False, SEEDS[17])
    short = _ref64(qkv[:, :16].contiguous(), do[:, :16].contiguous(), 2)
    for n in NAMES:
        bad = torch.nn.functional.pad(short[n], (0, 0, 0, 0, 0, 1))
        with pytest.raises(AssertionError, match="worst 16-row block"):
            _close_blocks(bad, ref[n], BF16_BOUNDS[n], BLOCK, 1, n)
        _close_blocks(ref[n], ref[n], BF16_BOUNDS[n], BLOCK, 1, n)


def test_selfcheck_self_scale():
    """T = 1: the float64 references of dQ and dK are exactly zero, the cancelling terms are not, and a dQ / dK that
    keeps one of those terms (delta dropped: dS = p dP) is rejected by the absolute bound."""
    for H, Hkv, hd in ((2, 2, 32), (2, 2, 128), (4, 2, 64)):
        qkv, do, _, _, ref, floor, zs = _case(2, 1, H, Hkv, hd, False, SEEDS[1])
        assert not ref["dq"].any() and not ref["dk"].any() and bool((zs["dq"] > 0).all()) and bool((zs["dk"] > 0).all())
        assert floor["dq"][1] <= 0.5 * G_TOL and floor["dk"][1] <= 0.5 * G_TOL
        _, q, k, v, dof = _heads(qkv, do, H, Hkv)
        k, v = (t.repeat_interleave(H // Hkv, 2) for t in (k, v))
        bad = (dof * v).sum(-1, keepdim=True) * hd ** -0.5 * k  # dQ without delta
        assert _figure("dq", bad, ref["dq"], zs)[1] > G_TOL


def test_selfcheck_spike_dq_decision():
    """SPIKE_DQ_OVER is what the float64 emulation of the bf16 rounding of O alone says at (1, 2048, 2, 128)."""
    B, T, H, hd = SPIKE
    qkv, do, ref, _ = _long(B, T, H, hd, True)
    worst, idx = _worst_block(_dq_o_rounding_alone(qkv, do, H), ref["dq"])
    print(f"SEQLEN-FLOOR | {SPIKE} spike | dq from the bf16 rounding of O alone {worst:.3e} at {idx}")
    assert (worst > G_TOL) == SPIKE_DQ_OVER, worst
