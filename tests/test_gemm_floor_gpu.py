"""fp32-output GEMMs at their fp32 floor, every kernel family of ``csrc/gemm.hip`` by name (docs/NUMERICS.md).

``_close(a, b, 2e-3)`` bounds an fp32 GEMM output about 1000x above what fp32 accumulation gives: one stray
bf16 rounding of a split-K slab, of the residual or of ``beta * dW`` passes it.  Here every output is checked
per element against ``T(K) * D`` with ``D = |A| . |B|`` (the componentwise scale of a dot product) and ``T(K)``
four times the error of a deliberately pessimistic CPU emulation of fp32 accumulation (:func:`_emulate`),
plus the rounding of the values the epilogue adds.  The factor 4 covers the MFMA's undocumented internal order
and the ordered slab sums; it is not tuned to any kernel's error.

Every case first asserts which family ran (``ops.gemm.last_launch``: the launch site's own record), so a
changed plan condition cannot move a case onto another kernel unnoticed.  References are float64 torch built
from the bf16-rounded inputs and from no kernel output (on the GPU where a CPU matmul would take seconds).

The ``test_selfcheck_*`` tests need no GPU.
"""

import contextlib
import functools

import pytest
import torch

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import gemm as G
from distributed_training_compare_jax_amd.ops.gemm import last_launch

gpu = pytest.mark.gpu

EPS_F32 = 2.0 ** -22   # fp32 epilogue: a few roundings (2^-24 each) of the values it adds
EPS_BF16 = 2.0 ** -8   # bf16 output: its unit roundoff (8 significant bits)
EPS_EXP = 2.0 ** -20   # v_exp / v_rcp of the GELU pair (about 1 ulp each, a few of them)
MARGIN = 4.0


# ------------------------------------------------------------------------------------------------ metrics

def _r(*shape, scale=1.0, seed=0):
    """The suite's generator (tests/test_kernels_gpu.py ``_r``): randn * scale + 0.1 rand, fp32 on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + 0.1 * torch.rand(*shape, generator=g)


def _bf64(t):
    return t.to(torch.bfloat16).double()


def _trunc32(x64):
    """float64 -> fp32 rounded toward zero, as float64."""
    y = x64.float()
    away = y.double().abs() > x64.abs()
    return torch.where(away, torch.nextafter(y, torch.zeros_like(y)), y).double()


def _emulate(a64, b64):
    """A pessimistic fp32 accumulation of a64 [m, K] . b64 [n, K]^T: exact blocks of 8 products, the running
    sum truncated toward zero to fp32 after each block (every rounding errs in the same direction)."""
    m, K = a64.shape
    n = b64.shape[0]
    nb = (K + 7) // 8
    pad = nb * 8 - K
    if pad:
        a64 = torch.nn.functional.pad(a64, (0, pad))
        b64 = torch.nn.functional.pad(b64, (0, pad))
    a3, b3 = a64.view(m, nb, 8), b64.view(n, nb, 8)
    acc = torch.zeros(m, n, dtype=torch.float64)
    for c0 in range(0, nb, 256):
        part = torch.einsum("mck,nck->cmn", a3[:, c0:c0 + 256], b3[:, c0:c0 + 256])
        for p in part:
            acc = _trunc32(acc + p)
    return acc


def _floor(a64, b64):
    """max_ij |emulation - exact| / D of one problem."""
    ref = a64 @ b64.t()
    d = a64.abs() @ b64.abs().t()
    return ((_emulate(a64, b64) - ref).abs() / d).max().item()


def _sub(K, scale_b):
    """The 96 x 80 sub-problem of the test generators at this K (bf16-rounded, float64)."""
    return _bf64(_r(96, K, seed=9001)), _bf64(_r(80, K, scale=scale_b, seed=9002))


@functools.lru_cache(maxsize=None)
def T(K, scale_b=0.05):
    """Componentwise tolerance of a K-long fp32 dot product: 4x the emulation's floor on the 96 x 80
    sub-problem of the test's generators (``scale_b``: 0.05 weights, 1.0 the activations of a weight gradient)."""
    return MARGIN * _floor(*_sub(K, scale_b))


def _bound_f32(ref, d, t, *added):
    b = t * d + EPS_F32 * ref.abs()
    for x in added:
        b = b + EPS_F32 * x.abs()
    return b


def _bound_bf16(ref, d, t, slope=None, extra=None):
    b = EPS_BF16 * ref.abs() + t * (d if slope is None else d * slope.abs()) + 1e-30
    return b if extra is None else b + extra


def _bound_colsum(dsum, beta_db0=None):
    b = 1e-6 * dsum
    return b if beta_db0 is None else b + EPS_F32 * beta_db0.abs()


def _within(out, ref, bound):
    o = out.double()
    return bool(torch.isfinite(o).all()) and bool(((o - ref).abs() <= bound).all())


def _check(out, ref, bound, name, d=None, floor=None):
    """Every element finite and within its bound; prints the worst err / bound (and, for fp32 outputs, the
    kernel's componentwise error over the emulation's)."""
    o = out.double()
    err = (o - ref).abs()
    ratio = err / bound
    worst = ratio.max().item()
    line = f"FLOOR-RATIO | {name} | err/bound {worst:.3f}"
    if d is not None and floor:
        comp = (err / d).max().item()
        line += f" | err/D {comp:.3e} | emulation {floor:.3e} | kernel/emulation {comp / floor:.2f}"
    print(line)
    assert bool(torch.isfinite(o).all()), f"{name}: {int((~torch.isfinite(o)).sum())} non-finite elements"
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(
            f"{name}: element {idx}: got {o.flatten()[i].item():.9e}, ref {ref.flatten()[i].item():.9e}, err "
            f"{err.flatten()[i].item():.3e} = {worst:.2f} x bound {bound.flatten()[i].item():.3e} "
            f"({int((ratio > 1).sum())} of {ratio.numel()} elements over)")


def _close_ok(a, b, rtol):
    """tests/test_kernels_gpu.py ``_close`` as a predicate."""
    return (a - b).abs().max().item() <= rtol * (b.abs().max().item() + 1e-6)


# K of every case below with the operand scales it is used at (0.05: x . W^T, dY . W; 1.0: dY^T . X)
KS = [(64, 0.05), (96, 0.05), (128, 0.05), (192, 0.05), (256, 0.05), (384, 0.05), (512, 0.05), (1024, 0.05),
      (16384, 0.05), (50304, 0.05), (96, 1.0), (512, 1.0), (1024, 1.0), (4096, 1.0), (8192, 1.0)]


# --------------------------------------------------------------------------------------- self-checks (CPU)

@pytest.mark.parametrize("K,scale_b", KS)
def test_selfcheck_tolerance_below_bf16_rounding(K, scale_b):
    """T(K) is at most a quarter of what the fp32 metric gives for a result rounded once to bf16."""
    a, b = _sub(K, scale_b)
    ref = a @ b.t()
    d = a.abs() @ b.abs().t()
    rounded = ((_bf64(ref) - ref).abs() / d).max().item()
    print(f"FLOOR-T | K {K} scale_b {scale_b} | floor {T(K, scale_b) / MARGIN:.3e} | T {T(K, scale_b):.3e} | "
          f"bf16-rounded result {rounded:.3e}")
    assert T(K, scale_b) <= rounded / 4, (K, scale_b, T(K, scale_b), rounded)
    assert not _within(_bf64(ref), ref, _bound_f32(ref, d, T(K, scale_b)))


def _selfcheck_problem(K, scale_b):
    a, b = _bf64(_r(192, K, seed=9011)), _bf64(_r(160, K, scale=scale_b, seed=9012))
    return a, b, a @ b.t(), a.abs() @ b.abs().t()


def test_selfcheck_rejects_bf16_slab():
    """One of four split-K slabs carried through bf16: accepted at 2e-3 of the maximum, rejected here."""
    K = 1024
    a, b, ref, d = _selfcheck_problem(K, 0.05)
    slabs = [a[:, i * 256:(i + 1) * 256] @ b[:, i * 256:(i + 1) * 256].t() for i in range(4)]
    wrong = slabs[0] + slabs[1] + _bf64(slabs[2]) + slabs[3]
    assert _close_ok(wrong, ref, 2e-3)
    assert _within(sum(slabs), ref, _bound_f32(ref, d, T(K)))
    assert not _within(wrong, ref, _bound_f32(ref, d, T(K)))


def test_selfcheck_rejects_bf16_residual():
    """The residual rounded to bf16 before the add."""
    K = 1024
    a, b, acc, d = _selfcheck_problem(K, 0.05)
    res = _r(192, 160, seed=9013).double()
    ref = acc + res
    wrong = acc + _bf64(res)
    assert _close_ok(wrong, ref, 2e-3)
    assert not _within(wrong, ref, _bound_f32(ref, d, T(K), res))


def test_selfcheck_rejects_dropped_accumulate():
    """beta * C0 with C0 = 0.01 randn dropped from a weight gradient."""
    K = 1024
    a, b, acc, d = _selfcheck_problem(K, 1.0)
    g = torch.Generator().manual_seed(9014)
    c0 = 0.01 * torch.randn(192, 160, generator=g, dtype=torch.float64)
    ref = acc + c0
    assert _close_ok(acc, ref, 2e-3)
    assert _within(ref.float(), ref, _bound_f32(ref, d, T(K, 1.0), c0))
    assert not _within(acc, ref, _bound_f32(ref, d, T(K, 1.0), c0))


# ------------------------------------------------------------------------------------------- GPU plumbing

def _g(t, dtype=torch.bfloat16):
    return t.to("cuda").to(dtype)


def _mm64(a, b):
    """(a . b, |a| . |b|) in float64 for bf16 / fp32 GPU operands a [m, k], b [k, n], results on the GPU: on the
    CPU when that takes about a second at most, else float64 torch on the GPU (vendor BLAS, not our kernels)."""
    m, k = a.shape
    n = b.shape[1]
    if m * n * k <= 3e8:
        a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
        return (a64 @ b64).cuda(), (a64.abs() @ b64.abs()).cuda()
    a64, b64 = a.double(), b.double()
    return a64 @ b64, a64.abs() @ b64.abs()


@contextlib.contextmanager
def _knob(name, value):
    """A ``dtc_gemm_set_*`` value for the duration of a block (restored in ``finally``)."""
    fn = getattr(N.lib(), "dtc_gemm_set_" + name)
    old = fn(value)
    try:
        yield
    finally:
        fn(old)


@contextlib.contextmanager
def _knobs(kv):
    with contextlib.ExitStack() as st:
        for k, v in kv.items():
            st.enter_context(_knob(k, v))
        yield


def _ran(expect, what):
    """The launch record matches ``expect`` (field -> value); asserted before any number."""
    torch.cuda.synchronize()
    ll = last_launch()
    for k, v in expect.items():
        assert getattr(ll, k) == v, f"{what}: expected {k} = {v!r}, the launch site recorded {ll}"
    return ll


def _gelu64(u):
    """float64 gelu(u), gelu'(u), gelu''(u)."""
    v = u.clone().requires_grad_(True)
    d = G.gelu_tanh_grad(v)
    (dd,) = torch.autograd.grad(d.sum(), v)
    return G.gelu_tanh(u), d.detach(), dd


DOMAIN = [0.0, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]


def _nt(M, Nn, K, ops, expect, knobs=None, seed=100):
    """y = x . W^T with the epilogues ``ops`` on one (M, N, K); every op on the family ``expect``."""
    tag = f"{expect['family']} NT {M}x{Nn}x{K}"
    x, w = _g(_r(M, K, seed=seed)), _g(_r(Nn, K, scale=0.05, seed=seed + 1))
    b = _g(_r(Nn, seed=seed + 2), torch.float32)
    acc, d = _mm64(x, w.t())
    b64 = b.double()
    t = T(K)
    fl = t / MARGIN
    with _knobs(knobs or {}):
        for op in ops:
            name = f"{tag} {op}"
            if op == "bf16":
                y = G.linear(x, w, b)
                _ran(expect, name)
                _check(y, acc + b64, _bound_bf16(acc + b64, d, t), name)
            elif op == "f32":
                y = G.linear(x, w, b, out_dtype=torch.float32)
                _ran(expect, name)
                _check(y, acc + b64, _bound_f32(acc + b64, d, t, b64.expand_as(acc)), name, d, fl)
            elif op == "f32_nobias":
                y = G.linear(x, w, out_dtype=torch.float32)
                _ran(expect, name)
                _check(y, acc, _bound_f32(acc, d, t), name, d, fl)
            elif op in ("resid", "resid_alias"):
                res = _g(_r(M, Nn, seed=seed + 3), torch.float32)
                r64 = res.double()
                y = G.linear_resid(x, w, b, res, out=res if op == "resid_alias" else None)
                _ran(expect, name)
                _check(y, acc + b64 + r64, _bound_f32(acc + b64 + r64, d, t, b64.expand_as(acc), r64), name, d, fl)
            elif op in ("gelu", "gelu_domain"):
                bias = b
                if op == "gelu_domain":  # both saturated tails and the range where exp2 overflows
                    bias = torch.tensor(DOMAIN, device="cuda").repeat((Nn + 8) // 9)[:Nn].contiguous()
                u = acc + bias.double()
                g64, d64, dd64 = _gelu64(u)
                dk, gk = G.linear_gelu(x, w, bias)
                _ran(expect, name)
                extra = EPS_EXP * (1 + u.abs())
                _check(gk, g64, _bound_bf16(g64, d, t, d64, extra), name + " g")
                _check(dk, d64, _bound_bf16(d64, d, t, dd64, extra), name + " d")
            elif op == "dgelu":
                uf = _g(_r(M, Nn, seed=seed + 4))
                y = G.matmul_nt_dgelu(x, w, uf)
                _ran(expect, name)
                _check(y, acc * uf.double(), _bound_bf16(acc * uf.double(), d, t, uf.double()), name)
            elif op == "f32_bias_refused":  # split-K slabs hold bare accumulators: a bias is an error, never dropped
                with pytest.raises(RuntimeError, match="1010"):
                    G.linear(x, w, b, out_dtype=torch.float32)
            else:
                raise AssertionError(op)


def _nn(M, Nn, K, ops, expect, knobs=None, seed=200):
    """dX [M, Nn] = dY [M, K] . W [K, Nn] (W the MN-major operand)."""
    tag = f"{expect['family']} NN {M}x{Nn}x{K}"
    dy, w = _g(_r(M, K, seed=seed)), _g(_r(K, Nn, scale=0.05, seed=seed + 1))
    acc, d = _mm64(dy, w)
    t = T(K)
    with _knobs(knobs or {}):
        for op in ops:
            name = f"{tag} {op}"
            if op == "f32":
                y = G.matmul_nn(dy, w)
                _ran(expect, name)
                _check(y, acc, _bound_f32(acc, d, t), name, d, t / MARGIN)
            elif op == "bf16":
                y = G.matmul_nn(dy, w, out_dtype=torch.bfloat16)
                _ran(expect, name)
                _check(y, acc, _bound_bf16(acc, d, t), name)
            elif op == "dgelu":
                uf = _g(_r(M, Nn, seed=seed + 2))
                y = G.matmul_nn_dgelu(dy, w, uf)
                _ran(expect, name)
                _check(y, acc * uf.double(), _bound_bf16(acc * uf.double(), d, t, uf.double()), name)
            else:
                raise AssertionError(op)


# accumulate semantics: (name, beta, C0 as a multiple of the reference's standard deviation; None = NaN prefill)
ACC = [("beta0_nan", 0.0, None), ("beta1_small", 1.0, 0.01), ("beta1_large", 1.0, 100.0)]


def _start(ref, mult, seed):
    """C0 of an accumulate case: mult * sigma(ref) * randn, or all NaN (beta = 0 must overwrite it)."""
    if mult is None:
        return torch.full(ref.shape, float("nan"), device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cpu").manual_seed(seed)
    sigma = ref.std().item() if ref.numel() > 1 else 1.0
    return (torch.randn(ref.shape, generator=g) * (mult * sigma)).to("cuda")


def _check_acc(dw, db, dw0, db0, beta, ref, d, cs, dsum, t, name):
    if beta:
        c = beta * dw0.double()  # (a large C0's own rounding dwarfs the product's: no kernel / emulation figure then)
        small = c.abs().max().item() <= ref.abs().max().item()
        _check(dw, ref + c, _bound_f32(ref + c, d, t, c), name + " dW", d if small else None, t / MARGIN)
    else:
        _check(dw, ref, _bound_f32(ref, d, t), name + " dW", d, t / MARGIN)
    if db is not None:
        cb = beta * db0.double() if beta else None
        _check(db, cs if cb is None else cs + cb, _bound_colsum(dsum, cb), name + " db")


def _tn(tokens, Nout, Kin, expect, with_db=False, use_red=False, knobs=None, seed=300):
    """dW [Nout, Kin] = beta dW + dY^T . X (+ db) in the three accumulate cases."""
    from distributed_training_compare_jax_amd.ops.reduce import GradReducer

    tag = f"{expect['family']} TN dW[{Nout},{Kin}] tokens {tokens}"
    dy, x = _g(_r(tokens, Nout, seed=seed)), _g(_r(tokens, Kin, seed=seed + 1))
    ref, d = _mm64(dy.t(), x)
    cs, dsum = dy.double().sum(0), dy.double().abs().sum(0)
    t = T(tokens, 1.0)
    red = GradReducer(torch.device("cuda"), arena_mb=64) if use_red else None
    with _knobs(knobs or {}):
        for i, (acc_name, beta, mult) in enumerate(ACC):
            dw0 = _start(ref, mult, seed + 10 + i)
            db0 = _start(cs, mult, seed + 20 + i) if with_db else None
            dw, db = dw0.clone(), None if db0 is None else db0.clone()
            G.wgrad(dy, x, dw, beta=beta, red=red, db=db)
            _ran(expect, f"{tag} {acc_name}")
            if red is not None:
                red.flush_all()
            _check_acc(dw, db, dw0, db0, beta, ref, d, cs, dsum, t, f"{tag} {acc_name}")


REG, DMA64, DMAW, BIG, R8, N8 = ("gemm_kernel", "gemm_dma_kernel", "gemm_dmaw_kernel", "gemm8p_kernel",
                                 "gemm8r_kernel", "gemm8n_kernel")
NT_ALL = ("bf16", "f32", "resid", "gelu", "dgelu")


# ------------------------------------------------------------------------------------------------ NT cases

NT_CASES = [
    # register-staged 64^2, BK 32 (K not a multiple of 64)
    ("reg64_bk32", 200, 136, 96, NT_ALL + ("gelu_domain",), dict(family=REG, bm=64, bn=64, sub=32, split_k=1), None),
    # gemm_dma_kernel 64^2 (NT, BK 64).  At (512, 768, 256) the bf16 epilogues belong to gemm8r by default
    ("dma64_f32", 512, 768, 256, ("f32", "resid"), dict(family=DMA64, bm=64, bn=64, split_k=1), None),
    ("dma64_all", 200, 136, 64, NT_ALL + ("gelu_domain",), dict(family=DMA64, bm=64, bn=64, split_k=1), None),
    # register-staged 128^2: M = 4096 is a multiple of 256 and goes to gemm8r; 4000 rows keep the 32 x 8 tiles
    ("reg128", 4000, 1024, 512, ("gelu", "gelu_domain", "dgelu"), dict(family=REG, bm=128, bn=128, sub=64), None),
    # gemm_dmaw_kernel 128 x 64
    ("dmaw", 1024, 1536, 128, ("resid", "f32", "bf16"), dict(family=DMAW, bm=128, bn=64, split_k=1), None),
    ("dmaw_ragged", 1000, 1544, 192, ("resid", "f32", "bf16"), dict(family=DMAW, bm=128, bn=64, split_k=1), None),
    # gemm8p whole tiles
    ("big_1round", 4096, 4096, 64, NT_ALL + ("gelu_domain",), dict(family=BIG, bm=256, bn=256, sub=4, split_k=1), None),
    ("big_wide", 2048, 16384, 64, NT_ALL, dict(family=BIG, bm=256, bn=256, sub=4, split_k=1), None),
    ("big_ragged", 2000, 16400, 128, NT_ALL, dict(family=BIG, bm=256, bn=256, sub=4, split_k=1), None),
    # gemm8p split-K, fp32 out
    ("big_splitk", 256, 256, 16384, ("f32_nobias", "f32_bias_refused"), dict(family=BIG, bm=256, bn=256, sub=4, split_k=32), None),
    ("big_splitk_ragged", 200, 264, 16384, ("f32_nobias",), dict(family=BIG, bm=256, bn=256, sub=4, split_k=32), None),
    # gemm8p 256 x 192 plan (128 blocks x split 2 = one per CU)
    ("big_cb3", 4096, 1536, 16384, ("f32_nobias",), dict(family=BIG, bm=256, bn=192, sub=3, split_k=2), None),
    # gemm8r, narrow tiles only: the plan gives CB2 = 1 whenever every width fits one round; CB2 = 2 and 4 need
    # more narrow tiles than CUs ((8192, 768) and (2048, 7936))
    ("r8_n64", 256, 64, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_n128", 256, 128, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_n256", 256, 256, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_n320", 256, 320, 256, ("bf16", "gelu", "gelu_domain", "dgelu", "f32"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_cb2", 8192, 768, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=2, aux=0), dict(r8=7)),
    ("r8_cb4", 2048, 7936, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=4, aux=0), dict(r8=7)),
    # gemm8r, mixed widths: columns 0..2047 on 256^2 tiles, the rest on 256 x 64
    ("r8_mixed", 8192, 2304, 256, ("bf16", "gelu", "dgelu", "f32"), dict(family=R8, sub=1, aux=2048), dict(r8=7)),
    # gemm8n, K = 1024: CB 3 (also ragged M) and CB 4
    ("n8_cb3", 8192, 768, 1024, NT_ALL + ("gelu_domain",), dict(family=N8, bm=128, bn=192, sub=3), None),
    ("n8_cb3_ragged", 8100, 768, 1024, NT_ALL, dict(family=N8, bm=128, bn=192, sub=3), None),
    ("n8_cb3_wide", 4096, 1536, 1024, NT_ALL, dict(family=N8, bm=128, bn=192, sub=3), None),
    ("n8_cb4", 8192, 1024, 1024, NT_ALL, dict(family=N8, bm=128, bn=256, sub=4), None),
]


@gpu
@pytest.mark.parametrize("name,M,Nn,K,ops,expect,knobs", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_floor_nt(cuda, name, M, Nn, K, ops, expect, knobs):
    _nt(M, Nn, K, ops, expect, knobs)


NN_ALL = ("f32", "bf16", "dgelu")
NN_CASES = [
    ("reg64_bk32", 256, 64, 96, NN_ALL, dict(family=REG, bm=64, bn=64, sub=32), None),
    ("reg64_bk64", 256, 128, 64, NN_ALL, dict(family=REG, bm=64, bn=64, sub=64, split_k=1), None),
    ("reg64_bk64_ragged", 300, 136, 64, NN_ALL, dict(family=REG, bm=64, bn=64, sub=64, split_k=1), None),
    ("big_splitk", 256, 256, 16384, ("f32",), dict(family=BIG, bm=256, bn=256, sub=4, split_k=32), None),
    ("r8_n64", 256, 64, 256, ("bf16", "dgelu"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_n320", 256, 320, 256, ("bf16", "dgelu"), dict(family=R8, sub=1, aux=0), dict(r8=7)),
    ("r8_mixed", 8192, 2304, 256, ("bf16", "dgelu"), dict(family=R8, sub=1, aux=2048), dict(r8=7)),
    ("n8_cb3", 8192, 768, 1024, NN_ALL, dict(family=N8, bm=128, bn=192, sub=3), None),
    ("n8_cb4", 8192, 1024, 1024, NN_ALL, dict(family=N8, bm=128, bn=256, sub=4), None),
]


@gpu
@pytest.mark.parametrize("name,M,Nn,K,ops,expect,knobs", NN_CASES, ids=[c[0] for c in NN_CASES])
def test_floor_nn(cuda, name, M, Nn, K, ops, expect, knobs):
    _nn(M, Nn, K, ops, expect, knobs)


# Weight gradients.  The register-staged TN plan is 64^2 only at BK 32 (make_plan sends every K % 64 == 0 weight
# gradient to 128^2 tiles), so there is no TN case on 64^2, BK 64.
TN_CASES = [
    ("reg64_bk32", 96, 136, 200, dict(family=REG, bm=64, bn=64, sub=32, split_k=1), False, False, None),
    ("reg64_bk32_db", 96, 136, 200, dict(family=REG, bm=64, bn=64, sub=32, split_k=1), True, True, None),
    ("reg128_splitk_db", 4096, 512, 512, dict(family=REG, bm=128, bn=128, sub=64, split_k=8), True, True, None),
    ("dmaw_256_t1024", 1024, 256, 256, dict(family=DMAW, bm=64, bn=128, split_k=2), False, False, None),
    ("dmaw_256_t8192", 8192, 256, 256, dict(family=DMAW, bm=64, bn=128, split_k=16), False, False, None),
    ("dmaw_768_t1024", 1024, 768, 768, dict(family=DMAW, bm=128, bn=128, split_k=2), False, False, None),
    ("dmaw_768_t8192", 8192, 768, 768, dict(family=DMAW, bm=128, bn=128, split_k=4), False, False, dict(wgrad256=0)),
    ("big_splitk_t8192", 8192, 768, 768, dict(family=BIG, bm=256, bn=256, sub=4, split_k=16), False, False, None),
    ("big_splitk_t8192_db", 8192, 768, 768, dict(family=BIG, bm=256, bn=256, sub=4, split_k=16), True, True, None),
    ("big_whole", 1024, 4096, 4096, dict(family=BIG, bm=256, bn=256, sub=4, split_k=1), False, False, None),
]


@gpu
@pytest.mark.parametrize("name,tokens,Nout,Kin,expect,with_db,use_red,knobs", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_floor_wgrad(cuda, name, tokens, Nout, Kin, expect, with_db, use_red, knobs):
    _tn(tokens, Nout, Kin, expect, with_db, use_red, knobs)


# ------------------------------------------------------------------------------------- the other launchers

@gpu
def test_floor_lmhead_logits(cuda):
    """gemm8p whole tiles with the LMHEAD epilogue (1576 tiles, ragged last N tile): the bf16 logits."""
    from distributed_training_compare_jax_amd.ops import xent as X

    M, Dm, V, Vp = 2048, 256, 50258, 50304
    h, w = _g(_r(M, Dm, seed=22)), _g(_r(Vp, Dm, scale=0.2, seed=23))
    b = _g(_r(Vp, seed=24), torch.float32)
    labels = torch.randint(0, V, (M,), dtype=torch.int32, generator=torch.Generator().manual_seed(25)).cuda()
    logits, _, _ = X.lmhead_logits_partials(h, w, b, labels, 0, V)
    _ran(dict(family=BIG, bm=256, bn=256, sub=4, split_k=1, epi=N.EPI_LMHEAD), "lm_head logits")
    acc, d = _mm64(h, w.t())
    ref = acc + b.double()
    t = MARGIN * _floor(_bf64(_r(96, Dm, seed=9001)), _bf64(_r(80, Dm, scale=0.2, seed=9002)))
    _check(logits[:, :V], ref[:, :V], _bound_bf16(ref, d, t)[:, :V], "gemm8p_kernel LMHEAD 2048x50304x256")
    assert bool((logits[:, V:] == float("-inf")).all())


@gpu
def test_floor_pair(cuda):
    """gemm_pair_kernel: dX, dW and db of one paired launch against float64 in the three accumulate cases."""
    from distributed_training_compare_jax_amd.ops.reduce import GradReducer

    M, Nout, Kin = 512, 384, 256
    dy, w, x = _g(_r(M, Nout, seed=41)), _g(_r(Nout, Kin, scale=0.05, seed=42)), _g(_r(M, Kin, seed=43))
    dx_ref, dx_d = _mm64(dy, w)
    ref, d = _mm64(dy.t(), x)
    cs, dsum = dy.double().sum(0), dy.double().abs().sum(0)
    red = GradReducer(torch.device("cuda"), arena_mb=64)
    for i, (acc_name, beta, mult) in enumerate(ACC):
        dw0, db0 = _start(ref, mult, 50 + i), _start(cs, mult, 60 + i)
        dw, db = dw0.clone(), db0.clone()
        dx = G.linear_backward(dy, w, x, dw, beta, red=red, db=db)
        _ran(dict(family="gemm_pair_kernel", bm=64, bn=128, split_k=1), f"pair {acc_name}")
        red.flush_all()
        name = f"gemm_pair_kernel {M}x{Nout}x{Kin} {acc_name}"
        _check(dx, dx_ref, _bound_f32(dx_ref, dx_d, T(Nout)), name + " dX", dx_d, T(Nout) / MARGIN)
        _check_acc(dw, db, dw0, db0, beta, ref, d, cs, dsum, T(M, 1.0), name)


GROUP_SHAPES = [(768, 3072), (3072, 768), (768, 768), (2304, 768), (200, 768), (384, 96)]  # test_wgrad_group_gpu.SHAPES
# 7 problems with a bias gradient (252 tiles) + one without (36): 288 tiles = one round of 256 + a tail of 32, all
# of it in the bias-free problem, which the launch sorts last
TAIL_SHAPES = [(768, 3072, True)] * 7 + [(3072, 768, False)]


def _group(shapes, tokens, expect, tag):
    t = T(tokens, 1.0)
    data = {}
    for (M, Nn, _) in shapes:  # problems of one shape share their operands and reference
        if (M, Nn) not in data:
            dy, x = _g(_r(tokens, M, seed=3 * M + Nn)), _g(_r(tokens, Nn, seed=3 * M + Nn + 1))
            data[(M, Nn)] = (dy, x, *_mm64(dy.t(), x), dy.double().sum(0), dy.double().abs().sum(0))
    for i, (acc_name, beta, mult) in enumerate(ACC):
        items, starts = [], []
        for j, (M, Nn, bias) in enumerate(shapes):
            dy, x, ref, d, cs, dsum = data[(M, Nn)]
            dw0 = _start(ref, mult, 1000 * i + 2 * j)
            db0 = _start(cs, mult, 1000 * i + 2 * j + 1) if bias else None
            starts.append((dw0, db0))
            items.append((dy, x, dw0.clone(), None if db0 is None else db0.clone()))
        G.wgrad_group(list(items), beta)
        _ran(expect, f"{tag} {acc_name}")
        for j, ((M, Nn, bias), (dy, x, dw, db), (dw0, db0)) in enumerate(zip(shapes, items, starts)):
            _, _, ref, d, cs, dsum = data[(M, Nn)]
            _check_acc(dw, db, dw0, db0, beta, ref, d, cs, dsum, t, f"{tag} {acc_name} problem {j} dW[{M},{Nn}]")


@gpu
def test_floor_wgrad_group(cuda):
    shapes = [(M, Nn, i % 2 == 0) for i, (M, Nn) in enumerate(GROUP_SHAPES)]
    _group(shapes, 1024, dict(family="gemm8p_group_kernel", sub=0, aux=113), "gemm8p_group_kernel")


@gpu
def test_floor_wgrad_group_tail_split(cuda):
    """Every problem of a launch whose last 32 tiles run as 4 K-pieces each, finished by wg_tail_reduce."""
    assert G._WG_TAIL == 1
    _group(TAIL_SHAPES, 1024, dict(family="gemm8p_group_kernel", sub=32, split_k=4, aux=288), "gemm8p_group_kernel tail")


@gpu
def test_floor_ce_dgrad(cuda):
    """ce_dgrad_fused's dx against the float64 product of its own bf16 dlogits and W^T."""
    from distributed_training_compare_jax_amd.ops import xent as X

    M, Dm, V, Vp = 512, 256, 1000, 1024
    g = torch.Generator().manual_seed(31)
    logits = (torch.randn(M, Vp, generator=g) * 3).to(torch.bfloat16)
    logits[:, V:] = float("-inf")
    logits = logits.cuda()
    lse = torch.logsumexp(logits.float(), -1).contiguous()
    labels = torch.randint(0, V, (M,), dtype=torch.int32, generator=g).cuda()
    wt = _g(_r(Dm, Vp, scale=0.05, seed=32))
    dx, dl, _ = X.ce_dgrad_fused(logits, lse, labels, 0, V, 1.0 / M, wt)
    _ran(dict(family="ce_dgrad256_kernel", bm=256, bn=256, split_k=1), "ce_dgrad_fused")
    dl64, wt64 = dl.cpu().double(), wt.cpu().double()
    ref, d = (dl64 @ wt64.t()).cuda(), (dl64.abs() @ wt64.abs().t()).cuda()
    t = MARGIN * _floor(dl64[:96], wt64[:80])  # the emulation on this operand pair: dlogits are no randn
    _check(dx, ref, _bound_f32(ref, d, t), "ce_dgrad256_kernel 512x256x1024 dx", d, t / MARGIN)


# ----------------------------------------------------------------------------------------- strided operands

def _sliced(t, pad=8):
    """``t`` as a column slice of a wider tensor whose other columns are NaN (ld > width, 16-byte aligned)."""
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), dtype=t.dtype, device=t.device)
    wide[:, pad:pad + t.shape[1]] = t
    return wide[:, pad:pad + t.shape[1]]


STRIDED = [
    ("nt_reg", "nt", 200, 136, 96, dict(family=REG, sub=32)),
    ("nt_dma64", "nt", 200, 136, 64, dict(family=DMA64)),
    ("nt_dmaw", "nt", 1024, 1536, 128, dict(family=DMAW, bm=128, bn=64)),
    ("nt_big", "nt", 4096, 4096, 64, dict(family=BIG, sub=4)),
    ("nn_reg", "nn", 300, 136, 64, dict(family=REG, sub=64)),
    ("tn_reg", "tn", 96, 136, 200, dict(family=REG, sub=32)),
]


@gpu
@pytest.mark.parametrize("name,layout,M,Nn,K,expect", STRIDED, ids=[c[0] for c in STRIDED])
def test_strided_operands_bitwise(cuda, name, layout, M, Nn, K, expect):
    """A and B as column slices of wider tensors (the lm_head chunks of models/gpt.py: ldb > K), NaN in the
    neighbouring columns: the same bits and the same kernel as on contiguous copies.  NT also with ``out``
    aliasing ``resid``."""
    if layout == "nt":
        a, b = _g(_r(M, K, seed=71)), _g(_r(Nn, K, scale=0.05, seed=72))
        bias = _g(_r(Nn, seed=73), torch.float32)
        res = _g(_r(M, Nn, seed=74), torch.float32)

        def run(a, b):
            r = res.clone()
            out = [G.linear(a, b, bias), G.linear(a, b, bias, out_dtype=torch.float32), G.linear_resid(a, b, bias, r, out=r)]
            lls = _ran(expect, name)
            return out, lls
    elif layout == "nn":
        a, b = _g(_r(M, K, seed=71)), _g(_r(K, Nn, scale=0.05, seed=72))

        def run(a, b):
            out = [G.matmul_nn(a, b), G.matmul_nn(a, b, out_dtype=torch.bfloat16)]
            return out, _ran(expect, name)
    else:  # M = tokens
        a, b = _g(_r(M, Nn, seed=71)), _g(_r(M, K, seed=72))

        def run(a, b):
            dw = torch.full((Nn, K), float("nan"), device="cuda")
            G.wgrad(a, b, dw, beta=0.0)
            return [dw], _ran(expect, name)
    want, ll0 = run(a, b)
    got, ll1 = run(_sliced(a), _sliced(b))
    assert ll0 == ll1
    for w_, g_ in zip(want, got):
        assert bool(torch.isfinite(w_).all())
        assert torch.equal(w_, g_), f"{name}: {int((w_ != g_).sum())} elements differ"
