"""Scale-aware numerics of the kernels whose outputs span decades: causal attention, the cross-entropy
backward and LayerNorm (docs/NUMERICS.md).

``test_kernels_gpu._close`` bounds ``max|a-b|`` by ``rtol * max|b|`` over the whole tensor.  For these three
families the few largest elements set that bound and the rest of the tensor goes unchecked: attention's late
query rows / last key rows are 10-100x smaller than row 0, 99.5 % of a cross-entropy gradient lies below 3e-2
of the label entry, and ``randn*3+1`` rows cannot tell a two-pass variance from ``E[x^2] - mean^2``.  Here the
same tolerances are applied per 16-row block (attention), per element (cross-entropy) and per row on rows with
a large mean (LayerNorm), always against a float64 reference that no kernel output feeds.

The three ``test_selfcheck_*`` tests need no GPU: they show on float64 data that each metric rejects a wrong
result that the global one accepts.
"""

import functools

import pytest
import torch

from test_kernels_gpu import _attn_ref64, _close, _r

from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.ops import layernorm as LN
from distributed_training_compare_jax_amd.ops import xent as X

gpu = pytest.mark.gpu

BLOCK = 16  # the smallest query-row / key-row granularity of any attention kernel (one 16x16 MFMA tile)


# ------------------------------------------------------------------------------------------------ metrics

def _block_ratios(out, ref64, block, dim):
    """Per (batch, head, block of ``block`` rows along ``dim``): max|out-ref| / max|ref|.  Tensors are
    [B, T, H, hd]-like: ``dim`` is the sequence axis, the last axis goes with the block's rows, every
    other axis (batch, head) stays separate.  A ragged last block holds the remaining rows."""
    err = (out.detach().cpu().double() - ref64).abs().movedim(dim, -2)
    ref = ref64.abs().movedim(dim, -2)
    T = err.shape[-2]
    pad = (-T) % block
    if pad:  # zeros change neither maximum
        err = torch.nn.functional.pad(err, (0, 0, 0, pad))
        ref = torch.nn.functional.pad(ref, (0, 0, 0, pad))
    lead = err.shape[:-2]
    err = err.reshape(*lead, (T + pad) // block, -1).amax(-1)
    ref = ref.reshape(*lead, (T + pad) // block, -1).amax(-1)
    return err, ref


def _worst_block(out, ref64, block=BLOCK, dim=1):
    err, ref = _block_ratios(out, ref64, block, dim)
    ratio = err / ref.clamp_min(1e-300)
    i = int(ratio.argmax())
    return ratio.flatten()[i].item(), tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))


def _close_blocks(out, ref64, rtol, block, dim, name):
    err, ref = _block_ratios(out, ref64, block, dim)
    worst, idx = _worst_block(out, ref64, block, dim)
    assert bool((err <= rtol * ref).all()), (
        f"{name}: worst {block}-row block (batch, head, block) = {idx}: max abs err / max |ref| = {worst:.3e} "
        f"> rtol {rtol:.1e} ({int((err > rtol * ref).sum())} of {err.numel()} blocks over)")


def _close_elem(out, ref64, rtol, atol, name):
    out64 = out.detach().cpu().double()
    err = (out64 - ref64).abs()
    over = err - (rtol * ref64.abs() + atol)
    i = int(over.argmax())
    assert over.flatten()[i].item() <= 0, (
        f"{name}: element {tuple(int(j) for j in torch.unravel_index(torch.tensor(i), err.shape))}: "
        f"got {out64.flatten()[i].item():.6e}, ref {ref64.flatten()[i].item():.6e}, err "
        f"{err.flatten()[i].item():.3e} > {rtol:.3e} * |ref| + {atol:.3e} ({int((over > 0).sum())} elements over)")


def _close_rows(out, ref64, rtol, name, rows=None):
    """``_close`` for every row on its own: max|out-ref| <= rtol * max|ref| within the row."""
    err = (out.detach().cpu().double() - ref64).abs().amax(-1)
    ref = ref64.abs().amax(-1)
    if rows is not None:
        err, ref = err[rows], ref[rows]
    ratio = err / ref.clamp_min(1e-300)
    i = int(ratio.argmax())
    assert bool((err <= rtol * ref).all()), (
        f"{name}: worst row {i if rows is None else int(torch.nonzero(rows)[i])}: max abs err / row max = "
        f"{ratio[i].item():.3e} > rtol {rtol:.1e} ({int((err > rtol * ref).sum())} of {err.numel()} rows over)")


# ---------------------------------------------------------------------------------------------- attention

def _bf(t):
    return t.to(torch.bfloat16).double()


def _attn_inputs(B, T, H, hd, spike):
    qkv = _r(B, T, 3 * H * hd, seed=40 if spike else 20, dev="cpu")
    if spike:  # one key mid-sequence scaled up: the running max jumps late, the rows after it are the small ones
        qkv.view(B, T, 3, H, hd)[:, T // 2 + 5, 1] *= 12.0
    do = _r(B, T, H * hd, seed=41 if spike else 21, dev="cpu")
    return qkv, do


def _attn_emulate(qkv, do, H):
    """The flash kernels' rounding steps in float64 torch: P and dS rounded to bf16 before their second
    matmul, outputs rounded to bf16, everything else exact.  The error of this against the exact reference
    is the floor a correct bf16 kernel sits on."""
    B, T, C3 = qkv.shape
    hd = C3 // (3 * H)
    q, k, v = qkv.double().view(B, T, 3, H, hd).unbind(2)
    dof = do.double().view(B, T, H, hd)
    s = torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5
    s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    o = _bf(torch.einsum("bhts,bshd->bthd", _bf(p), v))
    delta = (dof * o).sum(-1).permute(0, 2, 1)
    ds = p * (torch.einsum("bthd,bshd->bhts", dof, v) - delta[..., None]) * hd ** -0.5
    dv = _bf(torch.einsum("bhts,bthd->bshd", _bf(p), dof))
    dq = _bf(torch.einsum("bhts,bshd->bthd", _bf(ds), k))
    dk = _bf(torch.einsum("bhts,bthd->bshd", _bf(ds), q))
    return {"o": o, "dq": dq, "dk": dk, "dv": dv}


@functools.lru_cache(maxsize=None)
def _attn_case(B, T, H, hd, spike=False):
    """Inputs, float64 reference and the bf16 emulation's worst-block errors of one shape: computed once,
    shared by every test of that shape and never modified."""
    qkv, do = _attn_inputs(B, T, H, hd, spike)
    o, lse, dqkv = _attn_ref64(qkv, do, H)
    dq, dk, dv = dqkv.view(B, T, 3, H, hd).unbind(2)
    ref = {"o": o.view(B, T, H, hd), "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    emu = _attn_emulate(qkv, do, H)
    floor = {n: _worst_block(emu[n], ref[n])[0] for n in emu}
    return qkv, do, ref, floor


def _report(family, shape, spike, name, out, ref, floor):
    worst, idx = _worst_block(out, ref[name])
    print(f"SCALE-RATIO | {family} | {name} | {shape}{' spike' if spike else ''} | kernel {worst:.3e} at {idx} | "
          f"emulation {floor[name]:.3e} | ratio {worst / floor[name]:.2f}")


RES32 = [(1, 512, 2, 32), (1, 508, 3, 32)]                     # resident: T <= 512 and T % 4 == 0
CHUNK32 = [(1, 1024, 2, 32), (1, 1000, 2, 32), (1, 203, 3, 32)]  # chunked: T > 512 or T % 4 != 0 (203: odd T)
HD64 = [(1, 1024, 2, 64), (1, 1000, 2, 64), (1, 777, 3, 64)]
# the kernels each (kind, flags) case must launch, in order: asserted against A.last_launch() after the call
FF, BF = A.FwdFlags, A.BwdFlags
FWD_FAMILY = {("res32", 0): ("attn_fwd_res_kernel<32>",), ("res32", FF.PLAIN_WAVES): ("attn_fwd_res_kernel<32>",),
              ("chunk32", 0): ("attn_fwd_chunk_kernel<32>",), ("hd64", 0): ("attn_fwd5_kernel<64,3>",),
              ("hd64", FF.WPS2): ("attn_fwd5_kernel<64,2>",), ("hd64", FF.ROUND4): ("attn_fwd32_kernel<64>",),
              ("hd64", FF.CHUNK16): ("attn_fwd_chunk_kernel<64>",)}
BWD_FAMILY = {("res32", 0): ("attn_bwd_fused_kernel<32>",), ("res32", BF.TWO_ROUND): ("attn_bwd_res_kernel<32>",),
              ("chunk32", 0): ("attn_bwd_dq_chunk_kernel<32>", "attn_bwd_dkdv_chunk_kernel<32>"),
              ("hd64", 0): ("attn_delta_kernel<64>", "attn_bwd_merged32_kernel<64>"),
              ("hd64", BF.FORCE_MERGED): ("attn_delta_kernel<64>", "attn_bwd_merged32_kernel<64>"),
              ("hd64", BF.CHUNK16): ("attn_bwd_dq_chunk_kernel<64>", "attn_bwd_dkdv_chunk_kernel<64>")}


def _ran(direction, family, flags):
    """Asserts the record of the call just made; returns the label of its SCALE lines, from the record."""
    rec = A.last_launch()
    assert rec.direction == direction and rec.kernels == family, (rec, family)
    return " + ".join(rec.kernels) + (f", flags {int(flags)}" if flags else "")


def _cases(table):
    out = []
    for kind, shapes, flags in table:
        out += [pytest.param(s, kind, f, False, id=f"{'x'.join(map(str, s))}-{kind}-f{f}") for s in shapes for f in flags]
    return out


FWD_CASES = _cases([("res32", RES32, (0, 1)), ("chunk32", CHUNK32, (0,)), ("hd64", HD64, (0, 32, 16, 4))]) + [
    pytest.param(HD64[0], "hd64", f, True, id=f"1x1024x2x64-hd64-f{f}-spike") for f in (0, 16)]
# Finding (docs/NUMERICS.md): on the spike input the softmax of the late queries saturates on the spike key, so
# dS = P (dP - delta) cancels, and delta = rowsum(dO * O) is formed from the forward's bf16-rounded O
# (csrc/attention.hip attn_delta_kernel and the delta passes of the dQ kernels).  That rounding alone -- the float64
# emulation with every other step exact -- leaves 7.9e-2 of the block's maximum in dQ (6 of 128 blocks over 3e-2);
# with an fp32 O the same emulation gives 3.7e-3.  No backward kernel can do better on a bf16 O.
SPIKE_DQ = pytest.mark.xfail(strict=True, reason="delta = rowsum(dO * O) from the bf16-rounded O: 7.9e-2 per block in "
                             "the float64 emulation of that rounding alone (docs/NUMERICS.md)")
BWD_CASES = [pytest.param(*c.values, ("dq", "dk", "dv"), id=c.id) for c in
             _cases([("res32", RES32, (0, 1)), ("chunk32", CHUNK32, (0,)), ("hd64", HD64, (0, 8, 4))])] + [
    pytest.param(HD64[0], "hd64", 0, True, ("dk", "dv"), id="1x1024x2x64-hd64-f0-spike-dkdv"),
    pytest.param(HD64[0], "hd64", 0, True, ("dq",), id="1x1024x2x64-hd64-f0-spike-dq", marks=SPIKE_DQ)]


@gpu
@pytest.mark.parametrize("shape,kind,flags,spike", FWD_CASES)
def test_attention_fwd_blocks(cuda, shape, kind, flags, spike):
    """o per 16-query block at 2e-2 of the block's own maximum, lse to 1e-3 absolute, against the float64
    materialised softmax; prints the kernel's worst-block error over the bf16 emulation's."""
    B, T, H, hd = shape
    qkv, _, ref, floor = _attn_case(B, T, H, hd, spike)
    o, lse = A.attn_fwd(qkv.to(cuda), H, flags=flags)
    family = _ran("fwd", FWD_FAMILY[kind, flags], flags)
    o = o.view(B, T, H, hd)
    _report(family, shape, spike, "o", o, ref, floor)
    lse_err = (lse.cpu().double() - ref["lse"]).abs().max().item()
    print(f"SCALE-LSE | {family} | {shape}{' spike' if spike else ''} | max abs err {lse_err:.3e}")
    _close_blocks(o, ref["o"], 2e-2, BLOCK, 1, "o")
    assert lse_err <= 1e-3, f"lse: max abs err {lse_err:.3e} > 1e-3"


@gpu
@pytest.mark.parametrize("shape,kind,flags,spike,tensors", BWD_CASES)
def test_attention_bwd_blocks(cuda, shape, kind, flags, spike, tensors):
    """dQ per 16-query block, dK and dV per 16-key block at 3e-2 of the block's own maximum.  The kernels get
    the GPU forward's own o and lse, as in training; the reference is independent of both.

    The spike input's dQ is an expected failure (SPIKE_DQ above): measured 7.9e-2 on the GPU kernel as in the
    emulation, where the bf16 rounding of O accounts for all of it; its dK and dV are asserted."""
    B, T, H, hd = shape
    qkv, do, ref, floor = _attn_case(B, T, H, hd, spike)
    qkv_d, do_d = qkv.to(cuda), do.to(cuda)
    o, lse = A.attn_fwd(qkv_d, H)
    d = A.attn_bwd(qkv_d, o, lse, do_d, H, flags=flags).view(B, T, 3, H, hd)
    family = _ran("bwd", BWD_FAMILY[kind, flags], flags)
    outs = {n: d[:, :, "qkv".index(n[1])] for n in tensors}
    for n, t in outs.items():
        _report(family, shape, spike, n, t, ref, floor)
    for n, t in outs.items():
        _close_blocks(t, ref[n], 3e-2, BLOCK, 1, n)


def test_selfcheck_blocks_reject_a_zeroed_last_block():
    """float64 only: dV with its last 16 key rows zeroed passes the global metric at 3e-2 and fails per block;
    the bf16 emulation (a correct kernel's rounding) passes per block with room to spare."""
    B, T, H, hd = HD64[0]
    _, _, ref, floor = _attn_case(B, T, H, hd)
    bad = ref["dv"].clone()
    bad[:, T - BLOCK:] = 0
    _close(bad, ref["dv"], 3e-2, "dv, last block zeroed (global metric)")
    with pytest.raises(AssertionError, match="worst 16-row block"):
        _close_blocks(bad, ref["dv"], 3e-2, BLOCK, 1, "dv")
    _close_blocks(ref["dv"], ref["dv"], 3e-2, BLOCK, 1, "dv")
    assert max(floor.values()) < 1e-2, floor  # the floor leaves at least 2x headroom under 2e-2 / 3e-2
    late = ref["o"][:, T - BLOCK:].abs().amax().item()
    assert ref["o"][:, 0].abs().amax().item() >= 10 * late  # late rows are >= 10x smaller than row 0


# ------------------------------------------------------------------------------------------ cross-entropy

CE_RTOL = 2.0 ** -7   # bf16 round-to-nearest is <= 2^-8 relative; one more ulp for the fp32 exp
CE_ATOL = 2.0 ** -20  # x scale: cancellation in p - 1 at confident labels


def _ce_ref64(logits, lse, labels, vstart, V, scale):
    """(exp(logits - lse) - onehot inside the shard) * scale in float64; pad columns (logit -inf) are 0."""
    M = logits.shape[0]
    p = torch.exp(logits.cpu().double() - lse.cpu().double()[:, None])
    p[:, V:] = 0.0
    loc = labels.cpu().long() - vstart
    inside = (loc >= 0) & (loc < V)
    p[torch.arange(M)[inside], loc[inside]] -= 1.0
    return p * scale


@gpu
@pytest.mark.parametrize("src,M,D,V,Vp,vstart", [("lmhead", 256, 128, 1000, 1024, 0), ("randn", 256, 256, 50258, 50304, 0),
                                                 ("randn", 256, 256, 25129, 25152, 25129)])
def test_ce_backward_elementwise(cuda, src, M, D, V, Vp, vstart):
    """dlogits of ce_backward_inplace and of ce_dgrad_fused, element by element, against float64 on the
    kernel's own inputs (bf16 logits, fp32 lse); column partials against the column sums.  vstart > 0: a
    vocab-parallel shard with half of the labels outside it."""
    g = torch.Generator().manual_seed(61)
    labels = torch.randint(0, 2 * V if vstart else V, (M,), dtype=torch.int32, generator=g).to(cuda)
    if src == "lmhead":  # the lm_head kernel's bf16 logits (-inf pads), as in test_lmhead_ce
        h, w = _r(M, D, seed=22), _r(Vp, D, scale=0.2, seed=23)
        logits, _, _ = X.lmhead_logits_partials(h, w, _r(Vp, dtype=torch.float32, seed=24), labels, vstart, V)
    else:
        logits = (torch.randn(M, Vp, generator=g) * 3).to(torch.bfloat16)
        logits[:, V:] = float("-inf")
        logits = logits.to(cuda)
    assert bool(torch.isneginf(logits[:, V:]).all())
    lse = torch.logsumexp(logits.float(), -1).contiguous()
    scale = 1.0 / M
    ref = _ce_ref64(logits, lse, labels, vstart, V, scale)
    wt = _r(D, Vp, scale=0.05, seed=32)
    dx, dl, cp = X.ce_dgrad_fused(logits, lse, labels, vstart, V, scale, wt)
    ref_dl, ref_cp = X.ce_backward_inplace(logits.clone(), lse, labels, vstart, V, scale, colpart=True)
    plain = X.ce_backward_inplace(logits.clone(), lse, labels, vstart, V, scale)
    rel = ((ref_dl.cpu().double() - ref).abs() / ref.abs().clamp_min(CE_ATOL * scale)).max().item()
    print(f"SCALE-CE | {src} {(M, V, Vp, vstart)} | max err / max(|ref|, atol) = {rel:.3e} (2^-8 = {2.0 ** -8:.3e})")
    _close_elem(ref_dl, ref, CE_RTOL, CE_ATOL * scale, "ce_backward_inplace dlogits")
    _close_elem(dl, ref, CE_RTOL, CE_ATOL * scale, "ce_dgrad_fused dlogits")
    assert torch.equal(dl, ref_dl) and torch.equal(plain, ref_dl)
    assert bool((dl[:, V:] == 0).all()) and bool((ref_dl[:, V:] == 0).all())
    _close(dx, dl.double() @ wt.double().t(), 2e-3, "dx")
    # column partials: ce_backward_inplace sums the fp32 gradient before rounding, ce_dgrad_fused its bf16 dlogits
    for name, part, d in (("ce_backward_inplace", ref_cp, ref), ("ce_dgrad_fused", cp, dl.cpu().double())):
        err = (part.cpu().double().sum(0) - d.sum(0)).abs()
        bound = 1e-5 * d.abs().sum(0) + CE_ATOL * scale
        j = int((err - bound).argmax())
        assert bool((err <= bound).all()), f"{name} column partials: column {j}: err {err[j]:.3e} > {bound[j]:.3e}"


def test_selfcheck_elem_rejects_doubled_small_gradients():
    """float64 only: every non-label gradient with p < 0.01 doubled passes the global metric at 3e-2 (the
    label entry sets its scale) and fails element by element."""
    M, V, Vp = 256, 1000, 1024
    g = torch.Generator().manual_seed(31)
    logits = (torch.randn(M, Vp, generator=g) * 3).to(torch.bfloat16)
    logits[:, V:] = float("-inf")
    labels = torch.randint(0, V, (M,), dtype=torch.int32, generator=g)
    lse = torch.logsumexp(logits.float(), -1)
    ref = _ce_ref64(logits, lse, labels, 0, V, 1.0 / M)
    small = (ref > 0) & (ref < 0.01 / M)  # non-label entries (the label's is negative) with p < 0.01
    assert small.float().mean().item() > 0.9
    bad = torch.where(small, 2 * ref, ref)
    _close(bad, ref, 3e-2, "dlogits, small entries doubled (global metric)")
    with pytest.raises(AssertionError, match="elements over"):
        _close_elem(bad, ref, CE_RTOL, CE_ATOL / M, "dlogits")
    _close_elem(ref.to(torch.bfloat16), ref, CE_RTOL, CE_ATOL / M, "dlogits rounded to bf16")


# ---------------------------------------------------------------------------------------------- LayerNorm

LN_EPS = 1e-6
LN_ROWS = ((0.0, 1.0), (100.0, 0.1), (-30.0, 0.05), (1000.0, 1.0), (0.0, 1e-3))  # (c, s): x[m] = c + s * randn(D)


def _offset_rows(M, D, seed):
    """fp32 rows cycling over LN_ROWS: a residual stream that drifted away from 0.  Returns (x, c)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([LN_ROWS[m % len(LN_ROWS)][0] for m in range(M)])
    s = torch.tensor([LN_ROWS[m % len(LN_ROWS)][1] for m in range(M)])
    return c[:, None] + s[:, None] * torch.randn(M, D, generator=g), c


def _ln_ref64(x, g, b):
    x = x.detach().cpu().double()
    mean = x.mean(-1)
    rstd = torch.rsqrt((x - mean[:, None]).pow(2).mean(-1) + LN_EPS)
    xhat = (x - mean[:, None]) * rstd[:, None]
    return mean, rstd, xhat, xhat * g.cpu().double() + b.cpu().double()


def _y_rows(x):
    """Rows whose y is checked at 1e-2: those where an fp32 two-pass LayerNorm on the CPU keeps xhat within 1e-3
    of float64 -- a condition on the input alone."""
    x = x.detach().cpu()
    mean = x.mean(-1, keepdim=True)
    xhat = (x - mean) * torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + LN_EPS)
    return (xhat.double() - _ln_ref64(x, torch.ones(1), torch.zeros(1))[2]).abs().amax(-1) < 1e-3


def _check_rstd(rstd, ref64, name):
    rel = ((rstd.detach().cpu().double() - ref64).abs() / ref64).max().item()
    m = int(((rstd.detach().cpu().double() - ref64).abs() / ref64).argmax())
    assert rel <= 1e-4, f"{name}: rstd of row {m} (c, s = {LN_ROWS[m % len(LN_ROWS)]}) off by {rel:.3e} relative > 1e-4"
    return rel


def _check_ln_fwd(x, c, g, b, y, mean, rstd, name):
    """Per row: rstd to 1e-4 relative, mean to 1e-6 |c| + 1e-6, y to 1e-2 of the row's max where _y_rows allows."""
    mr, rr, _, yr = _ln_ref64(x, g, b)
    rel = _check_rstd(rstd, rr, name)
    merr = (mean.cpu().double() - mr).abs()
    mtol = 1e-6 * c.abs().double() + 1e-6
    m = int((merr - mtol).argmax())
    print(f"SCALE-LN | {name} | rstd rel err {rel:.3e} | mean err / tol {(merr / mtol).max().item():.3f}")
    assert bool((merr <= mtol).all()), f"{name}: mean of row {m} off by {merr[m]:.3e} > {mtol[m]:.3e}"
    rows = _y_rows(x)
    assert bool(rows[1::len(LN_ROWS)].all()), "the (100, 0.1) rows must be among the checked ones"
    _close_rows(y, yr, 1e-2, name + " y", rows)


def _ln_bwd_ref64(dy, x, g, mean, rstd, dres):
    """LayerNorm backward in float64 from the fp32 mean / rstd the kernel is given."""
    dy, g = dy.detach().cpu().double(), g.cpu().double()
    rstd = rstd.cpu().double()[:, None]
    xhat = (x.cpu().double() - mean.cpu().double()[:, None]) * rstd
    gdy = dy * g
    dx = (gdy - gdy.mean(-1, keepdim=True) - xhat * (gdy * xhat).mean(-1, keepdim=True)) * rstd
    if dres is not None:
        dx = dx + dres.cpu().double()
    return dx, (dy * xhat).sum(0), dy.sum(0)


@gpu
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_layernorm_offset_rows(cuda, D):
    """layernorm_fwd, add_layernorm_fwd (fp32 and bf16 d) and layernorm_bwd on rows with a large mean."""
    M = 256
    x, c = _offset_rows(M, D, seed=70)
    g, b = _r(D, dtype=torch.float32, seed=13), _r(D, dtype=torch.float32, seed=14)
    xd = x.to(cuda)
    y, mu, rs = LN.layernorm_fwd(xd, g, b, LN_EPS, torch.bfloat16)
    _check_ln_fwd(x, c, g, b, y, mu, rs, f"layernorm_fwd D={D}")
    # the residual add in the LayerNorm pass: the offset sits in resid, d is a layer's small update
    d = _r(M, D, dtype=torch.float32, seed=71, dev="cpu") * 0.01
    for dd in (d, d.to(torch.bfloat16)):
        want = dd.float() + x
        xs, (y2, mu2, rs2) = LN.add_layernorm_fwd(dd.to(cuda), xd, g, b, LN_EPS, torch.bfloat16)
        assert torch.equal(xs.cpu(), want)
        _check_ln_fwd(want, c, g, b, y2, mu2, rs2, f"add_layernorm_fwd {str(dd.dtype)[6:]} D={D}")
    # backward, from the forward's own mean / rstd (checked above)
    dy, dres = _r(M, D, seed=15), _r(M, D, dtype=torch.float32, seed=16)
    dg, db = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
    dxc = torch.empty(M, D, dtype=torch.bfloat16, device=cuda)
    dx = LN.layernorm_bwd(dy, xd, g, mu, rs, dres, dg, db, 0.0, out_c=dxc)
    dxr, dgr, dbr = _ln_bwd_ref64(dy, x, g, mu, rs, dres)
    _close_rows(dx, dxr, 1e-4, "layernorm_bwd dx")
    _close_rows(dxc, dxr, 1e-2, "layernorm_bwd dx bf16")
    _close(dg.cpu(), dgr, 1e-4, "layernorm_bwd dgamma")
    _close(db.cpu(), dbr, 1e-4, "layernorm_bwd dbeta")


@gpu
@pytest.mark.parametrize("M,D,K", [(128, 256, 64), (256, 1024, 128)])
def test_gemm_ln_fused_offset_rows(cuda, M, D, K):
    """The GEMM-fused LayerNorm epilogues (ops/ln_fused.py) with the offset rows in the residual stream: the
    forward's per-chunk mean / M2 combination and the backward's xhat must hold on a large mean."""
    from distributed_training_compare_jax_amd.ops import ln_fused as LF

    res, c = _offset_rows(M, D, seed=72)
    # a small update (|a W^T + b| ~ 1e-2), so that the rows keep the offsets' ratio of mean to spread
    a, w = _r(M, K, seed=31), (_r(D, K, scale=0.05, seed=32, dtype=torch.float32) * 0.04).to(torch.bfloat16)
    bias = _r(D, dtype=torch.float32, seed=33) * 0.01
    g, be = _r(D, dtype=torch.float32, seed=35), _r(D, dtype=torch.float32, seed=36)
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    sync = LF.LnSync(cuda, M, D, nsites=2, step=step)
    x, (y, mu, rs) = LF.linear_resid_ln(a, w, bias, res.to(cuda), g, be, LN_EPS, sync, site=0)
    torch.cuda.synchronize()
    sync.check()
    # x: two fp32 roundings of the sum (2^-23 |x|) + the worst-case fp32 accumulation error of the K products
    # and the bias add ((K + 1) 2^-24 (sum|a w| + |b|))
    xr = res.double() + a.cpu().double() @ w.cpu().double().t() + bias.cpu().double()
    mag = (a.cpu().double().abs() @ w.cpu().double().abs().t() + bias.cpu().double().abs()).max().item()
    _close_elem(x, xr, 2.0 ** -23, (K + 1) * 2.0 ** -24 * mag, "linear_resid_ln x")
    _check_ln_fwd(x.cpu(), c, g, be, y, mu, rs, f"linear_resid_ln {M}x{D}x{K}")
    # backward: dy = dY wt^T and the LayerNorm backward on the same rows, in one launch
    dY, wt = _r(M, K, seed=51), _r(D, K, scale=0.05, seed=52)
    dres = _r(M, D, dtype=torch.float32, seed=55)
    outs = [torch.zeros(D, device=cuda) for _ in range(3)]
    dx, dxc = LF.dgrad_ln_bwd(dY, wt, x, g, mu, rs, dres, outs[0], outs[1], 0.0, dbias=outs[2], sync=sync, site=1)
    torch.cuda.synchronize()
    sync.check()
    dy = dY.cpu().double() @ wt.cpu().double().t()
    dxr, dgr, dbr = _ln_bwd_ref64(dy, x, g, mu, rs, dres)
    _close_rows(dx, dxr, 1e-4, "dgrad_ln_bwd dx")
    _close_rows(dxc, dxr, 1e-2, "dgrad_ln_bwd dx bf16")
    _close(outs[0].cpu(), dgr, 1e-4, "dgrad_ln_bwd dgamma")
    _close(outs[1].cpu(), dbr, 1e-4, "dgrad_ln_bwd dbeta")
    _close(outs[2].cpu(), dxr.sum(0), 1e-4, "dgrad_ln_bwd dbias")


def test_selfcheck_rstd_rejects_one_pass_variance():
    """CPU only: E[x^2] - mean^2 in fp32 passes the rstd check on the old ``randn*3+1`` rows and fails it on
    the offset rows; the fp32 two-pass variance passes on both."""
    def one_pass(x):
        mean = x.mean(-1)
        return torch.rsqrt(((x * x).mean(-1) - mean * mean).clamp_min(0) + LN_EPS)

    def two_pass(x):
        return torch.rsqrt((x - x.mean(-1, keepdim=True)).pow(2).mean(-1) + LN_EPS)

    one = torch.ones(1)
    for D in (64, 768, 1024):
        old = _r(256, D, dtype=torch.float32, seed=12, dev="cpu") * 3 + 1
        new, _ = _offset_rows(256, D, seed=70)
        _check_rstd(one_pass(old), _ln_ref64(old, one, one)[1], "one-pass, old rows")
        _check_rstd(two_pass(old), _ln_ref64(old, one, one)[1], "two-pass, old rows")
        _check_rstd(two_pass(new), _ln_ref64(new, one, one)[1], "two-pass, offset rows")
        with pytest.raises(AssertionError, match="rstd of row"):
            _check_rstd(one_pass(new), _ln_ref64(new, one, one)[1], "one-pass, offset rows")
