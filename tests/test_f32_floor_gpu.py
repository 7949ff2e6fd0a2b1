"""The exact-fp32 kernels (``dtype: fp32``: csrc/gemm_f32.hip, csrc/attention_f32.hip, ``dtc_ce_bwd_f32`` and the
fp32 lm_head / CE epilogue) at the fp32 floor, per element and per block (docs/NUMERICS.md, "Exact fp32").

``tests/test_kernels_f32_gpu.py`` bounds ``max|a-b|`` by ``1e-5 * max|ref|`` over the whole tensor.  That leaves
attention's late key rows, the non-label cross-entropy gradients and every small GEMM output unchecked, and nothing
there says which tile or split-K variant of ``gemm_f32_kernel`` ran.  Here

* every GEMM case first asserts the launch site's own record (``ops.gemm.last_launch_f32``), then checks every element
  against ``T(K) D + 2^-22 (|ref| + |bias| + |res| + |beta C0|)`` with ``D = |A| . |B|`` and ``T(K)`` four times the
  error of :func:`_chain`, a pessimistic float64 emulation of the MFMA's k-ordered fma chain;
* the lm_head epilogue, the CE combine and ``dtc_ce_bwd_f32`` are checked per element / per column at four times the
  error of an fp32 torch emulation of the same formulas on the same inputs;
* attention is checked per (batch, head, 16 rows) at four times the worst block of :func:`_attn_emulate32`, an fp32
  emulation of the kernels' arithmetic (log2-domain online softmax over 32-key steps, P recomputed from the stored
  lse, delta from the fp32 O, every MFMA sum an ordered fma chain), on the same shape and input.

The factor 4 (``MARGIN``) covers the hardware's undocumented summation order, the ordered split-K slab sums and device
transcendentals at 1 - 2 ulp; it is not tuned to any kernel.  Every reference is float64 torch on the CPU built from
the kernel's own fp32 inputs; the CE backward's inputs are the kernel's logits and lse, as for the bf16 kernels.

The ``test_selfcheck_*`` tests need no GPU.
"""

import functools

import pytest
import torch

from test_gemm_floor_gpu import (ACC, DOMAIN, EPS_F32, MARGIN, _bound_f32, _check, _check_acc, _gelu64, _sliced, _start,
                                 _trunc32, _within)
from test_kernels_f32_gpu import _close as _close_whole
from test_kernels_f32_gpu import _r
from test_kernels_gpu import _attn_ref64
from test_kernels_scale_gpu import BLOCK, _attn_inputs, _ce_ref64, _close_blocks, _close_elem, _worst_block

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.ops import gemm as G
from distributed_training_compare_jax_amd.ops import xent as X

gpu = pytest.mark.gpu

F32_TINY = 2.0 ** -126  # the smallest normal fp32: the only absolute slack of a per-element relative check
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def _old_ok(out, ref64, rtol=1e-5):
    """tests/test_kernels_f32_gpu.py ``_close`` (max|a-b| <= rtol * max|ref| over the whole tensor) as a predicate."""
    try:
        _close_whole(out, ref64, rtol)
    except AssertionError:
        return False
    return True


def _bf64(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------ GEMM: the floor

def _chain(a64, b64):
    """a64 [m, K] . b64 [n, K]^T as v_mfma_f32_32x32x2_f32 is documented (csrc/gemm_f32.hip): every product exact
    (fp32 x fp32 fits float64), each rounded once into one k-ordered chain with no wider sum.  Pessimistic: the
    running sum is truncated toward zero to fp32 after every k step, so all K roundings err in one direction."""
    acc = torch.zeros(a64.shape[0], b64.shape[0], dtype=torch.float64)
    for k in range(a64.shape[1]):
        acc = _trunc32(acc + a64[:, k, None] * b64[None, :, k])
    return acc


def _sub(K, scale_b):
    """The 96 x 80 sub-problem of the test generators at this K (fp32 values as float64)."""
    return _r(96, K, seed=9001).double(), _r(80, K, scale=scale_b, seed=9002).double()


@functools.lru_cache(maxsize=None)
def _floor(K, scale_b=0.05):
    a, b = _sub(K, scale_b)
    return ((_chain(a, b) - a @ b.t()).abs() / (a.abs() @ b.abs().t())).max().item()


def T(K, scale_b=0.05):
    """Componentwise tolerance of a K-long fp32 fma chain: 4x the chain emulation's floor on the sub-problem
    (``scale_b``: 0.05 weights; 1.0 the activations of a weight gradient, K = tokens)."""
    return MARGIN * _floor(K, scale_b)


# slab length of the split-K cases below (the kernel's kps at that K); elsewhere the self-check cuts K in four
KPS = {(4096, 0.05): 256, (4100, 0.05): 272, (4356, 0.05): 272, (1000, 0.05): 352, (777, 1.0): 288, (4096, 1.0): 256}
# every K of a case below with the scale of its B operand
KS = [(20, 0.05), (36, 0.05), (48, 0.05), (64, 0.05), (96, 0.05), (100, 0.05), (136, 0.05), (256, 0.05), (1000, 0.05),
      (4096, 0.05), (4100, 0.05), (4356, 0.05), (96, 1.0), (777, 1.0), (4096, 1.0)]


def _slabs(a, b, K, scale_b):
    kps = KPS.get((K, scale_b), (K // 4 + 3) // 4 * 4)
    return [a[:, i:i + kps] @ b[:, i:i + kps].t() for i in range(0, K, kps)]


@pytest.mark.parametrize("K,scale_b", KS)
def test_selfcheck_gemm_bound_rejects_one_bf16_rounding(K, scale_b):
    """float64 only: the exact result rounded to fp32 and the chain emulation are within the bound; the result rounded
    once to bf16, and the sum of the slabs with the first one rounded to bf16, are not -- at every K of the cases."""
    a, b = _sub(K, scale_b)
    ref, d = a @ b.t(), a.abs() @ b.abs().t()
    t = T(K, scale_b)
    bound = _bound_f32(ref, d, t)
    slabs = _slabs(a, b, K, scale_b)
    slab_wrong = _bf64(slabs[0]) + sum(slabs[1:])
    comp = lambda w: ((w - ref).abs() / d).max().item()  # noqa: E731
    print(f"FLOOR-T | fp32 chain | K {K} scale_b {scale_b} | floor {t / MARGIN:.3e} | T {t:.3e} | bf16-rounded result "
          f"{comp(_bf64(ref)):.3e} | one bf16 slab of {len(slabs)} {comp(slab_wrong):.3e} | passes the old 1e-5: result "
          f"{_old_ok(_bf64(ref), ref)}, slab {_old_ok(slab_wrong, ref)}")
    assert _within(ref.float(), ref, bound)
    assert _within(sum(slabs), ref, bound)
    assert not _within(_bf64(ref), ref, bound)
    assert not _within(slab_wrong, ref, bound)


def test_selfcheck_old_metric_passes_a_bf16_slab_under_accumulate():
    """float64 only: a weight gradient over 4096 tokens accumulated (beta = 1) onto C0 = 100 sigma randn, the
    ``beta1_large`` case of the tests below, with one of its 16 slabs rounded to bf16: C0 sets the tensor's maximum,
    so the whole-tensor 1e-5 check passes; the per-element bound, whose C0 term is 2^-22 |C0|, does not."""
    K = 4096
    a, b = _sub(K, 1.0)
    acc, d = a @ b.t(), a.abs() @ b.abs().t()
    g = torch.Generator().manual_seed(9003)
    c0 = 100.0 * acc.std() * torch.randn(acc.shape, generator=g, dtype=torch.float64)
    slabs = _slabs(a, b, K, 1.0)
    ref, wrong = acc + c0, _bf64(slabs[0]) + sum(slabs[1:]) + c0
    bound = _bound_f32(ref, d, T(K, 1.0), c0)
    assert _old_ok(wrong, ref)
    assert _within(ref.float(), ref, bound)
    assert not _within(wrong, ref, bound)


# ------------------------------------------------------------------------------------------ GEMM: GPU cases

def _mm64(a, b):
    """(a . b, |a| . |b|) in float64 on the CPU from fp32 CPU operands a [m, k], b [k, n]; moved to the GPU, where
    the elementwise comparisons run."""
    a64, b64 = a.double(), b.double()
    return (a64 @ b64).cuda(), (a64.abs() @ b64.abs()).cuda()


def _ran(expect, what):
    """The launch record matches ``expect`` (field -> value); asserted before any number."""
    ll = G.last_launch_f32()
    for k, v in expect.items():
        assert getattr(ll, k) == v, f"{what}: expected {k} = {v!r}, the launch site recorded {ll}"
    return ll


_K0, _K1 = 0.7978845608028654, 0.044715


def _gelu_bounds(u, bias64, d, t):
    """Reference and bounds of the fp32 GELU pair at the float64 pre-activation ``u`` (CPU autograd, results on the
    GPU).  ``du`` is the pre-activation's own bound; it enters through the slope (g' for g, g'' for d), second order
    ``du^2`` (|g''|, |g'''| < 2).  The epilogue's tanhf errs by ``eth`` = 2 ulp (2^-23) plus the four roundings of
    its argument, 2^-22 |inner| (1 - th^2); g = u (1 + th) / 2 and d = (1 + th) / 2 + u (1 - th^2) inner' / 2 take
    it with the factors |u| / 2 and 1 / 2 + |u th| inner'; the remaining roundings are 2^-22 of the terms summed."""
    g64, d64, dd64 = (x.cuda() for x in _gelu64(u.cpu()))
    du = t * d + EPS_F32 * (u.abs() + bias64.abs())
    inner, dinner = _K0 * (u + _K1 * u ** 3), _K0 * (1 + 3 * _K1 * u * u)
    th = torch.tanh(inner)
    eth = 2.0 ** -23 + 2.0 ** -22 * inner.abs() * (1 - th * th)
    t1, t2 = 0.5 * (1 + th), 0.5 * u * (1 - th * th) * dinner
    bg = du * d64.abs() + du * du + EPS_F32 * g64.abs() + 0.5 * u.abs() * eth
    bd = du * dd64.abs() + du * du + EPS_F32 * (t1.abs() + t2.abs()) + (0.5 + (u * th).abs() * dinner) * eth
    return g64, d64, bg, bd


def _nt(M, Nn, K, ops, expect, seed=100):
    """y = x . W^T with the epilogues ``ops`` on one (M, N, K), every op on the variant ``expect``."""
    tag = f"gemm_f32 {expect['bm']}x{expect['bn']} NT {M}x{Nn}x{K}"
    x, w, b = _r(M, K, seed=seed), _r(Nn, K, scale=0.05, seed=seed + 1), _r(Nn, seed=seed + 2)
    acc, d = _mm64(x, w.t())
    xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
    b64 = bc.double()
    t = T(K)
    fl = t / MARGIN
    expect = dict(expect, layout=0)
    for op in ops:
        name = f"{tag} {op}"
        if op == "nobias":
            y = G.linear(xc, wc)
            _ran(dict(expect, epi=N.EPI_STORE), name)
            _check(y, acc, _bound_f32(acc, d, t), name, d, fl)
        elif op == "bias":
            y = G.linear(xc, wc, bc)
            _ran(dict(expect, epi=N.EPI_STORE), name)
            _check(y, acc + b64, _bound_f32(acc + b64, d, t, b64.expand_as(acc)), name, d, fl)
        elif op == "resid":
            res = _r(M, Nn, seed=seed + 3).cuda()
            r64 = res.double()
            y = G.linear_resid(xc, wc, bc, res)
            _ran(dict(expect, epi=N.EPI_RESID), name)
            _check(y, acc + b64 + r64, _bound_f32(acc + b64 + r64, d, t, b64.expand_as(acc), r64), name, d, fl)
        elif op == "gelu_domain":  # both saturated tails: a bias cycling over 0, +-3, +-6, +-12, +-40 by column
            bias = torch.tensor(DOMAIN, device="cuda").repeat((Nn + 8) // 9)[:Nn].contiguous()
            bias64 = bias.double().expand_as(acc)
            g64, d64, bg, bd = _gelu_bounds(acc + bias64, bias64, d, t)
            dk, gk = G.linear_gelu(xc, wc, bias)
            _ran(dict(expect, epi=N.EPI_GELU), name)
            assert dk.dtype == torch.float32 and gk.dtype == torch.float32
            _check(gk, g64, bg, name + " g")
            _check(dk, d64, bd, name + " d")
        else:
            raise AssertionError(op)


def _nn(M, Nn, K, ops, expect, seed=200):
    """dX [M, Nn] = dY [M, K] . W [K, Nn] (W the N-major operand)."""
    tag = f"gemm_f32 {expect['bm']}x{expect['bn']} NN {M}x{Nn}x{K}"
    dy, w = _r(M, K, seed=seed), _r(K, Nn, scale=0.05, seed=seed + 1)
    acc, d = _mm64(dy, w)
    dyc, wc = dy.cuda(), w.cuda()
    t = T(K)
    expect = dict(expect, layout=1)
    for op in ops:
        name = f"{tag} {op}"
        if op == "plain":
            y = G.matmul_nn(dyc, wc)
            _ran(dict(expect, epi=N.EPI_STORE), name)
            _check(y, acc, _bound_f32(acc, d, t), name, d, t / MARGIN)
        elif op == "dgelu":
            uf = _r(M, Nn, seed=seed + 2).cuda()
            u64 = uf.double()
            y = G.matmul_nn_dgelu(dyc, wc, uf)
            _ran(dict(expect, epi=N.EPI_DGELU), name)
            assert y.dtype == torch.float32
            _check(y, acc * u64, _bound_f32(acc * u64, d * u64.abs(), t), name, d * u64.abs(), t / MARGIN)
        else:
            raise AssertionError(op)


def _tn(tokens, Nout, Kin, expect, seed=300):
    """dW [Nout, Kin] = beta dW + dY^T . X and db = beta db + colsum(dY) in the three accumulate cases."""
    tag = f"gemm_f32 {expect['bm']}x{expect['bn']} TN dW[{Nout},{Kin}] tokens {tokens}"
    dy, x = _r(tokens, Nout, seed=seed), _r(tokens, Kin, seed=seed + 1)
    ref, d = _mm64(dy.t(), x)
    cs, dsum = dy.double().sum(0).cuda(), dy.double().abs().sum(0).cuda()
    dyc, xc = dy.cuda(), x.cuda()
    t = T(tokens, 1.0)
    expect = dict(expect, layout=2, epi=N.EPI_STORE)
    for i, (acc_name, beta, mult) in enumerate(ACC):
        dw0, db0 = _start(ref, mult, seed + 10 + i), _start(cs, mult, seed + 20 + i)
        dw, db = dw0.clone(), db0.clone()
        G.wgrad(dyc, xc, dw, beta=beta, db=db)
        _ran(expect, f"{tag} {acc_name}")
        _check_acc(dw, db, dw0, db0, beta, ref, d, cs, dsum, t, f"{tag} {acc_name}")


T128 = dict(bm=128, bn=128, bk=16, split=1, split_off=0)
T128X64 = dict(bm=128, bn=64, bk=32, split=1, split_off=0)
T64 = dict(bm=64, bn=64, bk=32, split=1, split_off=0)


def _off(tile, K):
    """The plan asked for split-K and the epilogue switched it off: one pass over all of K."""
    return dict(tile, split=1, kps=K, split_off=1)


# (256, 256, 4100) runs 16 slabs of 272: its last slab is 20 long, one k-tile of 16 and a ragged one of 4.  A last slab
# shorter than a k-tile needs 17 slabs: (256, 256, 4356), 16 x 272 + 4.
NT_CASES = [
    ("t128_k20", 4096, 2048, 20, ("bias", "resid", "gelu_domain"), dict(T128, kps=20)),
    ("t128_k100", 4096, 2048, 100, ("bias", "resid", "gelu_domain"), dict(T128, kps=100)),
    ("t128x64_k36", 4096, 1024, 36, ("bias", "resid"), dict(T128X64, kps=36)),
    ("t64_first_loop_k48", 4096, 512, 48, ("bias", "resid"), dict(T64, kps=48)),
    ("t64_small", 200, 136, 96, ("nobias", "bias", "resid", "gelu_domain"), dict(T64, kps=96)),
    ("splitk128", 256, 256, 4096, ("nobias",), dict(T128, split=16, kps=256)),
    ("splitk128_ragged_tile", 256, 256, 4100, ("nobias",), dict(T128, split=16, kps=272)),
    ("splitk128_short_slab", 256, 256, 4356, ("nobias",), dict(T128, split=17, kps=272)),
    ("splitk64_ragged_slab", 128, 64, 1000, ("nobias",), dict(T64, split=3, kps=352)),
    ("split_off128", 256, 256, 4096, ("bias", "resid"), _off(T128, 4096)),
    ("split_off128_ragged", 256, 256, 4100, ("bias", "resid"), _off(T128, 4100)),
    ("split_off128_short", 256, 256, 4356, ("bias", "resid"), _off(T128, 4356)),
    ("split_off64", 128, 64, 1000, ("bias", "resid"), _off(T64, 1000)),
]


@gpu
@pytest.mark.parametrize("name,M,Nn,K,ops,expect", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_f32_floor_nt(cuda, name, M, Nn, K, ops, expect):
    _nt(M, Nn, K, ops, expect)


NN_CASES = [
    ("t128_k20", 4096, 2048, 20, ("plain", "dgelu"), dict(T128, kps=20)),
    ("t128_k100", 4096, 2048, 100, ("plain", "dgelu"), dict(T128, kps=100)),
    ("t64_first_loop_k48", 4096, 512, 48, ("plain",), dict(T64, kps=48)),
    ("t64_small", 300, 64, 136, ("plain", "dgelu"), dict(T64, kps=160)),
    ("splitk128", 256, 256, 4096, ("plain",), dict(T128, split=16, kps=256)),
    ("splitk128_ragged_tile", 256, 256, 4100, ("plain",), dict(T128, split=16, kps=272)),
    ("splitk128_short_slab", 256, 256, 4356, ("plain",), dict(T128, split=17, kps=272)),
    ("splitk64_ragged_slab", 128, 64, 1000, ("plain",), dict(T64, split=3, kps=352)),
    ("split_off128_dgelu", 256, 256, 4096, ("dgelu",), _off(T128, 4096)),
]


@gpu
@pytest.mark.parametrize("name,M,Nn,K,ops,expect", NN_CASES, ids=[c[0] for c in NN_CASES])
def test_f32_floor_nn(cuda, name, M, Nn, K, ops, expect):
    _nn(M, Nn, K, ops, expect)


TN_CASES = [
    ("splitk128", 4096, 256, 256, dict(T128, split=16, kps=256)),
    ("splitk64_ragged", 777, 96, 160, dict(T64, split=3, kps=288)),
    ("t64_nosplit", 96, 136, 200, dict(T64, kps=96)),
]


@gpu
@pytest.mark.parametrize("name,tokens,Nout,Kin,expect", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_f32_floor_wgrad(cuda, name, tokens, Nout, Kin, expect):
    _tn(tokens, Nout, Kin, expect)


@gpu
@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_f32_strided_operands_bitwise(cuda, layout):
    """A and B as column slices of wider tensors with NaN in the neighbouring columns (ld > width): the same bits
    and the same variant as on contiguous copies.  NT at K = 100 (a ragged last k-tile next to the NaN), TN split-K."""
    if layout == "nt":
        a, b = _r(200, 100, seed=71).cuda(), _r(136, 100, scale=0.05, seed=72).cuda()
        bias, res = _r(136, seed=73).cuda(), _r(200, 136, seed=74).cuda()

        def run(a, b):
            out = [G.linear(a, b, bias), G.linear_resid(a, b, bias, res)]
            return out, _ran(dict(T64, kps=128, layout=0), "strided nt")
    else:
        a, b = _r(777, 96, seed=71).cuda(), _r(777, 160, seed=72).cuda()

        def run(a, b):
            dw = torch.full((96, 160), float("nan"), device="cuda")
            G.wgrad(a, b, dw, beta=0.0)
            return [dw], _ran(dict(T64, split=3, kps=288, layout=2), "strided tn")
    want, ll0 = run(a, b)
    got, ll1 = run(_sliced(a), _sliced(b))
    assert ll0 == ll1
    for w_, g_ in zip(want, got):
        assert bool(torch.isfinite(w_).all())
        assert torch.equal(w_, g_), f"{layout}: {int((w_ != g_).sum())} elements differ"


# ---------------------------------------------------------------- lm_head epilogue, CE combine, CE backward

LM_SHAPES = [(256, 64, 990, 1024, 0), (256, 256, 25129, 25152, 25129), (256, 256, 50258, 50304, 0)]
LM_EXPECT = {990: T64, 25129: T128X64, 50258: T128}


@functools.lru_cache(maxsize=None)
def _lm_case(M, D, V, Vp, vstart):
    """Inputs and the float64 logits (pad columns -inf) of one lm_head shape: computed once, never modified."""
    h, w, b = _r(M, D, seed=12), _r(Vp, D, scale=0.05, seed=13), _r(Vp, seed=14)
    g = torch.Generator().manual_seed(15)
    labels = torch.randint(0, 2 * V if vstart else V, (M,), generator=g, dtype=torch.int32)
    ref = h.double() @ w.double().t() + b.double()
    ref[:, V:] = float("-inf")
    return h, w, b, labels, ref


def _lse_emulate32(h, w, b, V):
    """The epilogue's and the combine's formula in fp32 torch: fp32 logits, (max, sum exp) per 32-column wave slice
    (a slice of padding gives (-inf, 0)), lse = max + log sum_p s_p exp(m_p - max)."""
    logits = h @ w.t() + b
    logits[:, V:] = float("-inf")
    sl = logits.view(logits.shape[0], -1, 32)
    mp = sl.amax(-1)
    mpz = torch.where(mp > float("-inf"), mp, torch.zeros_like(mp))  # a dead slice: exp(-inf - 0) = 0, s_p = 0
    sp = torch.exp(sl - mpz[..., None]).sum(-1)
    mx = mp.amax(-1)
    return mx + torch.log((sp * torch.exp(mpz - mx[:, None])).sum(-1))


def _ce_emulate32(logits, lse, labels, vstart, V, scale):
    """common.h ``ce_grad8f`` in fp32 torch on the CPU: g = exp2(fma(l, log2 e, cr)) with cr = log2(scale) - lse log2 e,
    pad columns 0, the label's entry minus scale.  (The fma is formed in float64 and rounded once.)"""
    f = torch.float32
    l2e = torch.tensor(LOG2E, dtype=f)
    cr = torch.log2(torch.tensor(scale, dtype=f)) - lse.to(f) * l2e
    g = torch.exp2((logits.double() * l2e.double() + cr.double()[:, None]).to(f))
    g[:, V:] = 0.0
    loc = labels.long() - vstart
    inside = (loc >= 0) & (loc < V)
    g[torch.arange(g.shape[0])[inside], loc[inside]] -= torch.tensor(scale, dtype=f)
    return g


def _chunk_sums32(g, rows):
    """Column sums over chunks of ``rows`` rows, each an fp32 sum in row order (the kernel's loop)."""
    out = []
    for m0 in range(0, g.shape[0], rows):
        acc = torch.zeros(g.shape[1], dtype=torch.float32)
        for m in range(m0, min(m0 + rows, g.shape[0])):
            acc = acc + g[m]
        out.append(acc)
    return torch.stack(out)


def _ce_floors(logits, lse, labels, vstart, V, scale, rows):
    """(float64 reference, rtol of the gradient, rtol of the column partials against sum_m |d_mj|): 4x the worst
    element of the fp32 emulation on these inputs."""
    ref = _ce_ref64(logits, lse, labels, vstart, V, scale)
    emu = _ce_emulate32(logits, lse, labels, vstart, V, scale)
    nz = ref != 0
    rel = ((emu.double() - ref).abs()[nz] / ref.abs()[nz]).max().item()
    refc = torch.stack([ref[m0:m0 + rows].sum(0) for m0 in range(0, ref.shape[0], rows)])
    absc = torch.stack([ref[m0:m0 + rows].abs().sum(0) for m0 in range(0, ref.shape[0], rows)])
    live = absc > 0
    relc = ((_chunk_sums32(emu, rows).double() - refc).abs()[live] / absc[live]).max().item()
    return ref, refc, absc, MARGIN * rel, MARGIN * relc


@gpu
@pytest.mark.parametrize("M,D,V,Vp,vstart", LM_SHAPES, ids=[f"V{s[2]}_vstart{s[4]}" for s in LM_SHAPES])
def test_f32_lmhead_ce(cuda, M, D, V, Vp, vstart):
    """fp32 lm_head logits + (max, sum exp) partials, the combine's lse, the label logit and ``dtc_ce_bwd_f32`` with
    its column partials.  V = 990: columns 992..1023 are a whole wave slice of padding (its partial is (-inf, 0));
    vstart > 0: a vocab-parallel shard with half of the labels outside it."""
    h, w, b, labels, ref = _lm_case(M, D, V, Vp, vstart)
    hc, wc, bc, lc = h.cuda(), w.cuda(), b.cuda(), labels.cuda()
    name = f"lm_head {(M, D, V, Vp, vstart)}"
    single = vstart == 0
    logits, stat, labl = X.lmhead_logits_partials(hc, wc, bc, lc, vstart, V, combine=not single)
    _ran(dict(LM_EXPECT[V], layout=0, epi=N.EPI_LMHEAD), name)
    assert logits.dtype == torch.float32
    if single:
        lse, _ = X.ce_finalize(stat, labl, 1.0 / M)
        width = Vp // stat.shape[0]  # columns per partial: one wave's slice of the tile
        dead = stat[(V + width - 1) // width:]  # slices that hold padding only
        assert (dead.shape[0] > 0) == (V == 990)
        assert bool((dead[..., 0] == float("-inf")).all()) and bool((dead[..., 1] == 0).all())
    else:
        lse, _ = X.ce_finalize(stat.unsqueeze(0).contiguous(), labl, 1.0 / M)
    # logits at the GEMM bound, pad columns exactly -inf
    d = (h.double().abs() @ w.double().abs().t()).cuda()
    refc, b64 = ref.cuda(), b.double().cuda().expand(M, Vp)
    t = T(D)
    bound = _bound_f32(refc[:, :V], d[:, :V], t, b64[:, :V])
    _check(logits[:, :V], refc[:, :V], bound, name + " logits", d[:, :V], t / MARGIN)
    assert bool((logits[:, V:] == float("-inf")).all())
    # the label's logit: the stored logit itself where the label is inside the shard, 0 elsewhere
    loc = labels.long() - vstart
    inside = (loc >= 0) & (loc < V)
    assert bool(inside.any()) and (single or bool((~inside).any()))
    rows = torch.arange(M)
    lab_cpu, log_cpu = labl.cpu(), logits.cpu()
    assert torch.equal(lab_cpu[inside], log_cpu[rows[inside], loc[inside]])
    if not single:
        assert bool((lab_cpu[~inside] == 0).all())
    # lse, absolute, at 4x the fp32 emulation's error on these inputs
    lse_ref = torch.logsumexp(ref, -1)
    lse_tol = MARGIN * (_lse_emulate32(h, w, b, V).double() - lse_ref).abs().max().item()
    lse_err = (lse.cpu().double() - lse_ref).abs().max().item()
    print(f"F32-LSE | {name} | max abs err {lse_err:.3e} | emulation {lse_tol / MARGIN:.3e} | ratio "
          f"{lse_err * MARGIN / lse_tol:.2f}")
    assert lse_err <= lse_tol, f"lse: max abs err {lse_err:.3e} > {lse_tol:.3e}"
    # the backward, per element, against float64 on the kernel's own logits and lse
    scale = 1.0 / M
    R = int(N.lib().dtc_ce_colsum_rows())
    lse_cpu = lse.cpu()
    gref, refcol, abscol, rtol, rtol_col = _ce_floors(log_cpu, lse_cpu, labels, vstart, V, scale, R)
    dl, cp = X.ce_backward_inplace(logits.clone(), lse, lc, vstart, V, scale, colpart=True)
    dl_cpu, cp_cpu = dl.cpu(), cp.cpu().double()
    nz = gref != 0
    rel = ((dl_cpu.double() - gref).abs()[nz] / gref.abs()[nz]).max().item()
    colerr = (cp_cpu - refcol).abs()
    live = abscol > 0
    relc = (colerr[live] / abscol[live]).max().item()
    print(f"F32-CE | {name} | dlogits max rel err {rel:.3e} | emulation {rtol / MARGIN:.3e} | ratio "
          f"{rel * MARGIN / rtol:.2f} | column partials {relc:.3e} | emulation {rtol_col / MARGIN:.3e} | ratio "
          f"{relc * MARGIN / rtol_col:.2f}")
    _close_elem(dl_cpu, gref, rtol, F32_TINY, "dtc_ce_bwd_f32 dlogits")
    assert bool((dl_cpu[:, V:] == 0).all()) and bool((cp_cpu[:, V:] == 0).all())
    assert tuple(cp_cpu.shape) == tuple(refcol.shape)
    over = colerr - (rtol_col * abscol + F32_TINY)
    j = int(over.argmax())
    assert over.flatten()[j].item() <= 0, (
        f"column partials: (chunk, column) {divmod(j, Vp)}: err {colerr.flatten()[j].item():.3e} > "
        f"{rtol_col:.3e} * sum|d| = {(rtol_col * abscol).flatten()[j].item():.3e} ({int((over > 0).sum())} over)")


def test_selfcheck_ce_elementwise_rejects_a_uniform_relative_error():
    """float64 only, lm_head logits at V = 50258 (D = 64: the median gradient is 1.1e-5 of the label's, the largest
    non-label probability 4e-3): every non-label gradient scaled by 1.002 passes the whole-tensor 1e-5 (the label
    entry, about 1 / M, sets the maximum) and fails per element; so does the result rounded to bf16."""
    M, D, V, Vp, vstart = 256, 64, 50258, 50304, 0
    _, _, _, labels, logits64 = _lm_case(M, D, V, Vp, vstart)
    logits, lse = logits64.float(), torch.logsumexp(logits64, -1).float()
    ref, _, _, rtol, rtol_col = _ce_floors(logits, lse, labels, vstart, V, 1.0 / M, 128)
    print(f"FLOOR-T | ce_bwd_f32 {(M, V)} | dlogits rtol {rtol:.3e} | column partials rtol {rtol_col:.3e} | median |d| / "
          f"max |d| {(ref[:, :V].abs().median() / ref.abs().max()).item():.2e}")
    assert rtol <= 2.0 ** -10 and rtol_col <= 2.0 ** -10  # a quarter of a bf16 rounding at the most
    _close_elem(ref.float(), ref, rtol, F32_TINY, "dlogits rounded to fp32")
    bad = torch.where(ref > 0, 1.002 * ref, ref)  # the label's entry is the negative one
    assert _old_ok(bad, ref)
    with pytest.raises(AssertionError, match="elements over"):
        _close_elem(bad, ref, rtol, F32_TINY, "dlogits")
    with pytest.raises(AssertionError, match="elements over"):
        _close_elem(ref.to(torch.bfloat16), ref, rtol, F32_TINY, "dlogits rounded to bf16")


# ---------------------------------------------------------------------------------------------- attention

def _round32_(x64, buf32):
    """x64 (float64) rounded in place to the nearest fp32: one rounding step of an fp32 chain."""
    buf32.copy_(x64)
    x64.copy_(buf32)


def _dot_chain32(a64, b64):
    """a [n, T, hd] . b [n, S, hd]^T -> [n, T, S] as the kernels' MFMAs form S = Q K^T and dP = dO V^T: one fp32 fma
    chain over head_dim per element, rounded after every step (fp32 values as float64: every product is exact, so
    each step is one rounding to fp32)."""
    at, bt = a64.permute(2, 0, 1).contiguous(), b64.permute(2, 0, 1).contiguous()
    acc = torch.zeros(a64.shape[0], a64.shape[1], b64.shape[1], dtype=torch.float64)
    buf = torch.empty(acc.shape, dtype=torch.float32)
    for d in range(a64.shape[-1]):
        acc.addcmul_(at[d, :, :, None], bt[d, :, None, :])
        _round32_(acc, buf)
    return acc


def _attn_emulate32(qkv, do, H):
    """csrc/attention_f32.hip's arithmetic on the CPU, fp32 values (held as float64 where a fused multiply-add has
    to be rounded once).  Every MFMA sum is what the kernel header documents: each product rounded once into one
    ordered fma chain with no wider sum -- over head_dim for S = Q K^T and dP = dO V^T, over the keys in order for
    O += P V and dQ += dS K, over the queries in order for dV += P^T dO and dK += dS^T Q.  (A float32 matmul sums in
    vector lanes and blocks: at T = 1024 its chains are 15 to 30 times shorter and its O about twice as accurate as a
    one-accumulator sum's, and on the spike input dQ inherits the rounding of O through delta 300-fold.)
    Forward: scores times scale * log2(e), an online maximum over 32-key steps, exp2, the running sum and O rescaled
    by exp2(m_old - m_new), O times 1 / l, lse = (m + log2 l) ln 2.  Backward: P = exp2(fma(s, scale log2 e, -lse
    log2 e)) from the stored lse, delta = rowsum(dO * O) from the fp32 O, dS = P (dP - delta), dK and dQ scaled at
    the end.  A masked P is 0, and fma(acc, 0, x) = acc: the chains run over whole rows."""
    f, f64 = torch.float32, torch.float64
    B, T, C3 = qkv.shape
    hd = C3 // (3 * H)
    n = B * H
    q, k, v = (t.permute(0, 2, 1, 3).reshape(n, T, hd).double() for t in qkv.view(B, T, 3, H, hd).unbind(2))
    dof = do.view(B, T, H, hd).permute(0, 2, 1, 3).reshape(n, T, hd).double()
    scale = torch.tensor(hd ** -0.5, dtype=f)
    sc2 = scale * torch.tensor(LOG2E, dtype=f)
    idx = torch.arange(T)
    m = torch.full((n, T), float("-inf"), dtype=f)
    l = torch.zeros(n, T, dtype=f)
    o = torch.zeros(n, T, hd, dtype=f64)
    qk = _dot_chain32(q, k)  # the forward's S^T and the backward's S are the same chains
    for kb in range(0, T, 32):  # queries before kb see none of these keys
        ke = min(kb + 32, T)
        s = qk[:, kb:, kb:ke].to(f) * sc2
        s = s.masked_fill(idx[None, kb:ke] > idx[kb:, None], float("-inf"))
        m_new = torch.maximum(m[:, kb:], s.amax(-1))
        alpha = torch.exp2(m[:, kb:] - m_new)
        p = torch.exp2(s - m_new[..., None])
        l[:, kb:] = l[:, kb:] * alpha + p.sum(-1)
        m[:, kb:] = m_new
        ob, p = o[:, kb:], p.double()
        buf = torch.empty(ob.shape, dtype=f)
        ob.mul_(alpha.double()[..., None])
        _round32_(ob, buf)
        for j in range(kb, ke):
            ob.addcmul_(p[:, :, j - kb, None], v[:, j, None, :])
            _round32_(ob, buf)
    o = (o * (1.0 / l).double()[..., None]).to(f)
    lse = (m + torch.log2(l)) * torch.tensor(LN2, dtype=f)
    lse2 = lse * torch.tensor(LOG2E, dtype=f)
    delta = (dof.to(f) * o).sum(-1)
    p = torch.exp2((qk * sc2.double() - lse2.double()[..., None]).to(f))
    p = p.masked_fill(idx[None, :] > idx[:, None], 0.0)
    ds = (p * (_dot_chain32(dof, v) - delta.double()[..., None]).to(f)).double()
    p = p.double()
    # step j of the three chains: key j into dQ of every query, query j into dV and dK of every key
    mult = torch.stack([ds.permute(2, 0, 1), p.permute(1, 0, 2), ds.permute(1, 0, 2)], 1).contiguous()  # [T, 3, n, T]
    vec = torch.stack([k, dof, q]).permute(2, 0, 1, 3).contiguous()                                   # [T, 3, n, hd]
    acc = torch.zeros(3, n, T, hd, dtype=f64)
    buf = torch.empty(acc.shape, dtype=f)
    for j in range(T):
        acc.addcmul_(mult[j, :, :, :, None], vec[j, :, :, None, :])
        _round32_(acc, buf)
    out = {"o": o, "dq": acc[0].to(f) * scale, "dv": acc[1].to(f), "dk": acc[2].to(f) * scale}
    return {name: t.view(B, H, T, hd).permute(0, 2, 1, 3) for name, t in out.items()}, lse.view(B, H, T)


@functools.lru_cache(maxsize=None)
def _attn_case32(B, T, H, hd, spike=False):
    """fp32 inputs, float64 reference and the fp32 emulation's floors (worst 16-row block per tensor, worst lse) of
    one shape: computed once, shared and never modified."""
    if spike:
        qkv, do = (t.float() for t in _attn_inputs(B, T, H, hd, True))
    else:
        qkv, do = _r(B, T, 3 * H * hd, seed=16), _r(B, T, H * hd, seed=17)
    o, lse, dqkv = _attn_ref64(qkv, do, H)
    dq, dk, dv = dqkv.view(B, T, 3, H, hd).unbind(2)
    ref = {"o": o.view(B, T, H, hd), "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    emu, emu_lse = _attn_emulate32(qkv, do, H)
    floor = {n: _worst_block(emu[n], ref[n])[0] for n in emu}
    floor["lse"] = (emu_lse.double() - lse).abs().max().item()
    return qkv, do, ref, floor


ATTN_SHAPES = [(1, 1024, 2, 64), (1, 1000, 2, 64), (2, 200, 3, 32), (1, 520, 2, 32), (1, 72, 1, 128), (1, 777, 2, 128)]
ATTN_CASES = [pytest.param(s, False, id="x".join(map(str, s))) for s in ATTN_SHAPES] + [
    pytest.param(s, True, id="x".join(map(str, s)) + "-spike") for s in ((1, 1024, 2, 64), (1, 1024, 2, 128))]
ATTN_KERNEL = {"o": "attn_f32_fwd_kernel", "dq": "attn_f32_dq_kernel", "dk": "attn_f32_dkdv_kernel",
               "dv": "attn_f32_dkdv_kernel"}


@gpu
@pytest.mark.parametrize("shape,spike", ATTN_CASES)
def test_f32_attention_blocks(cuda, shape, spike):
    """o, dQ, dK, dV per (batch, head, 16 rows) at 4x the emulation's worst block of the same shape, input and tensor;
    lse absolute at 4x the emulation's.  The backward gets the GPU forward's own fp32 o and lse, as in training; the
    reference is independent of both.  The spike input's dQ is asserted: delta comes from an fp32 O here.  Its floor is
    not the plain one (docs/NUMERICS.md, "Exact fp32", finding): measured 2.45e-5 (head_dim 64) and 1.68e-4 (head_dim
    128) of the block's maximum, 1.00 and 0.88 of the emulation, against 1e-6 to 2e-6 on the other inputs."""
    B, T, H, hd = shape
    qkv, do, ref, floor = _attn_case32(B, T, H, hd, spike)
    qkv_d, do_d = qkv.to(cuda), do.to(cuda)
    o, lse = A.attn_fwd(qkv_d, H)
    assert o.dtype == torch.float32 and lse.shape == (B, H, T)
    d = A.attn_bwd(qkv_d, o, lse, do_d, H).view(B, T, 3, H, hd)
    outs = {"o": o.view(B, T, H, hd), "dq": d[:, :, 0], "dk": d[:, :, 1], "dv": d[:, :, 2]}
    tag = f"{shape}{' spike' if spike else ''}"
    for n, t in outs.items():
        worst, idx = _worst_block(t, ref[n])
        print(f"F32-RATIO | {ATTN_KERNEL[n]}<{hd}> | {n} | {tag} | kernel {worst:.3e} at {idx} | emulation "
              f"{floor[n]:.3e} | ratio {worst / floor[n]:.2f}")
    lse_err = (lse.cpu().double() - ref["lse"]).abs().max().item()
    print(f"F32-LSE | attn_f32_fwd_kernel<{hd}> | {tag} | max abs err {lse_err:.3e} | emulation {floor['lse']:.3e} | "
          f"ratio {lse_err / floor['lse']:.2f}")
    for n, t in outs.items():
        _close_blocks(t, ref[n], MARGIN * floor[n], BLOCK, 1, n)
    assert lse_err <= MARGIN * floor["lse"], f"lse: max abs err {lse_err:.3e} > {MARGIN * floor['lse']:.3e}"


def test_selfcheck_attention_blocks_reject_a_scaled_last_block():
    """float64 only, (1,1024,2,64): dV with its last 16 key rows scaled by 1 + 1e-3 passes the whole-tensor 1e-5 and
    fails per block at 4x the fp32 floor; the fp32 floors themselves lie below 1e-5 / 4."""
    B, T, H, hd = ATTN_SHAPES[0]
    _, _, ref, floor = _attn_case32(B, T, H, hd)
    print("FLOOR-T | attention fp32 emulation | " + str((B, T, H, hd)) + " | " +
          " | ".join(f"{n} {v:.3e}" for n, v in floor.items()))
    assert max(floor.values()) < 1e-5 / MARGIN, floor
    bad = ref["dv"].clone()
    bad[:, T - BLOCK:] *= 1.0 + 1e-3
    assert _old_ok(bad, ref["dv"])
    with pytest.raises(AssertionError, match="worst 16-row block"):
        _close_blocks(bad, ref["dv"], MARGIN * floor["dv"], BLOCK, 1, "dv")
    _close_blocks(ref["dv"].float(), ref["dv"], MARGIN * floor["dv"], BLOCK, 1, "dv rounded to fp32")
