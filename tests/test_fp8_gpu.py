"""The FP8 (e4m3) kernels of ``csrc/gemm_fp8.hip`` (docs/NUMERICS.md "FP8 forward").

A. The quantiser against the torch CPU path (the definition), bitwise: bytes and scale; the batched form against
   the single form.
B. The GEMM on the block-scaled MFMA.  Every case first asserts which variant ran (``last_launch_fp8``: the
   launch site's own record).
   B1: small-integer operands that e4m3 holds exactly; the fp32 output equals the integer product bitwise.
   B2: per element against ``T * D`` with ``D = |A| . |B|``, the conventions of ``tests/test_gemm_floor_gpu.py``
   (its helpers are copied here, not imported).  The reference is the float64 product of the DEQUANTISED operands,
   so quantisation error is not in the bound, and ``T`` is four times the floor of a pessimistic emulation of
   the accumulation, evaluated on the test's own dequantised operands.  The emulation models what the exact-data
   probe of the block-scaled MFMA shows (:func:`_emulate`): plain fp32 accumulation does not describe it (the
   kernel's err / D is 1.5e-5 at K = 128, about 350 times the fp32 emulation's 4.2e-8).
"""

import pytest
import torch

from distributed_training_compare_jax_amd.ops import fp8 as F
from distributed_training_compare_jax_amd.ops import gemm as G

gpu = pytest.mark.gpu

EPS_F32 = 2.0 ** -22   # fp32 epilogue: a few roundings (2^-24 each) of the values it adds
EPS_BF16 = 2.0 ** -8   # bf16 output: its unit roundoff (8 significant bits)
EPS_EXP = 2.0 ** -20   # v_exp / v_rcp of the GELU pair (about 1 ulp each, a few of them)
MARGIN = 4.0
V64, V128 = "fp8_64x128", "fp8_128x128"


def _r(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + 0.1 * torch.rand(*shape, generator=g)


def _trunc32(x64):
    """float64 -> fp32 rounded toward zero, as float64."""
    y = x64.float()
    away = y.double().abs() > x64.abs()
    return torch.where(away, torch.nextafter(y, torch.zeros_like(y)), y).double()


def _trunc_bits(x64, bits):
    """float64 cut toward zero to ``bits`` significant bits."""
    e = torch.floor(torch.log2(x64.abs().clamp_min(1e-300)))
    q = torch.exp2(e - (bits - 1))
    return torch.where(x64 == 0, x64, torch.trunc(x64 / q) * q)


ACC_BITS = 20   # significant bits of the running sum after a k-step (docs/NUMERICS.md)
MFMA_KEEP = 13  # bits kept below the largest product exponent of a 32-element block (docs/NUMERICS.md)


def _emulate(a64, b64):
    """A pessimistic model of the kernel's accumulation of a64 [m, K] . b64 [n, K]^T (K a multiple of 128), from the
    exact-data probe of the single instruction (benchmarks/mfma_f8_sum_probe.hip, docs/NUMERICS.md "FP8 forward"):
    within each 32-element block of k the exact products are aligned to the block's largest product exponent
    E = max_k (floor(log2 |a_k|) + floor(log2 |b_k|)) and cut toward zero to multiples of 2^(E - 13); the blocks'
    sums are exact; after every 128-long step the running sum is cut toward zero to 20 significant bits (the probe's
    accumulator cases come back rounded to 2^-19 of the accumulator at the coarsest; every cut here errs in the same
    direction, as in tests/test_gemm_floor_gpu.py)."""
    m, K = a64.shape
    n = b64.shape[0]
    assert K % 128 == 0
    expo = lambda t: torch.where(t == 0, torch.full_like(t, -200.0), torch.floor(torch.log2(t.abs().clamp_min(1e-300))))
    ea, eb = expo(a64), expo(b64)
    acc = torch.zeros(m, n, dtype=torch.float64)
    for k0 in range(0, K, 128):
        step = torch.zeros(m, n, dtype=torch.float64)
        for c0 in range(k0, k0 + 128, 32):
            prod = a64[:, None, c0:c0 + 32] * b64[None, :, c0:c0 + 32]
            e = (ea[:, None, c0:c0 + 32] + eb[None, :, c0:c0 + 32]).amax(-1).clamp_min(-200.0)
            q = torch.exp2(e - MFMA_KEEP)[..., None]
            step = step + (torch.trunc(prod / q) * q).sum(-1)
        acc = _trunc_bits(acc + step, ACC_BITS)
    return acc


def _floor(a64, b64):
    """max_ij |emulation - exact| / D of one problem."""
    ref = a64 @ b64.t()
    d = a64.abs() @ b64.abs().t()
    return ((_emulate(a64, b64) - ref).abs() / d).max().item()


def _bound_f32(ref, d, t, *added):
    b = t * d + EPS_F32 * ref.abs()
    for x in added:
        b = b + EPS_F32 * x.abs()
    return b


def _bound_bf16(ref, d, t, slope=None, extra=None):
    b = EPS_BF16 * ref.abs() + t * (d if slope is None else d * slope.abs()) + 1e-30
    return b if extra is None else b + extra


def _check(out, ref, bound, name, d=None, floor=None):
    """Every element finite and within its bound; prints the worst err / bound first."""
    o = out.double().cpu()
    err = (o - ref).abs()
    ratio = err / bound
    worst = ratio.max().item()
    line = f"FP8-FLOOR | {name} | err/bound {worst:.3f}"
    if d is not None and floor:
        comp = (err / d).max().item()
        line += f" | err/D {comp:.3e} | emulation {floor:.3e} | kernel/emulation {comp / floor:.2f}"
    print(line)
    assert bool(torch.isfinite(o).all()), f"{name}: {int((~torch.isfinite(o)).sum())} non-finite elements"
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: flat element {i}: got {o.flatten()[i].item():.9e}, ref {ref.flatten()[i].item():.9e}, "
                             f"err {err.flatten()[i].item():.3e} = {worst:.2f} x bound {bound.flatten()[i].item():.3e} "
                             f"({int((ratio > 1).sum())} of {ratio.numel()} elements over)")


def _gelu64(u):
    v = u.clone().requires_grad_(True)
    d = G.gelu_tanh_grad(v)
    (dd,) = torch.autograd.grad(d.sum(), v)
    return G.gelu_tanh(u), d.detach(), dd


def _cuda(t: F.Fp8Tensor) -> F.Fp8Tensor:
    return F.Fp8Tensor(t.q.cuda(), t.scale.cuda(), t.inv.cuda())


def _ran(variant, epilogue, out_f32, what):
    torch.cuda.synchronize()
    ll = F.last_launch_fp8()
    assert (ll.variant, ll.epilogue, ll.out_f32) == (variant, epilogue, out_f32), \
        f"{what}: expected {(variant, epilogue, out_f32)}, the launch site recorded {ll}"
    assert ll.tile == ((64, 128) if variant == V64 else (128, 128))


# -------------------------------------------------------------------------------------------- A: quantiser

def _quant_inputs(shape, dtype):
    """name -> tensor of ``shape``: the classes of values on which a quantiser can go wrong."""
    M, K = shape
    n = M * K
    g = torch.Generator().manual_seed(1000 * M + K)
    out = {}
    out["decades"] = torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, K, generator=g) * 9 - 6)
    sub = torch.randn(M, K, generator=g) * 2e-5  # amax 1 -> s = 256: these land in the e4m3 subnormal range
    sub.view(-1)[n // 2] = 1.0
    out["subnormal_range"] = sub
    # exact ties at s = 1 (amax 256): odd multiples of half a step in several binades and in the subnormal range
    steps = torch.tensor([2.0 ** -9] * 8 + [2.0 ** -9, 2.0 ** -8, 2.0 ** -6, 2.0 ** -3, 1.0, 2.0, 4.0, 16.0])
    base = torch.tensor([0., 1., 2., 3., 4., 5., 6., 7.] + [8., 9., 10., 11., 12., 13., 14., 15.])
    ties = (base + 0.5) * steps
    t = torch.cat([ties, -ties]).repeat(n // 32 + 1)[:n].reshape(M, K).clone()
    t.view(-1)[n - 1] = 256.0
    out["ties"] = t
    out["zero"] = torch.zeros(M, K)
    p = torch.rand(M, K, generator=g) * 2 - 1
    p.view(-1)[0] = -4.0  # amax exactly a power of two
    out["amax_pow2"] = p
    e = torch.rand(M, K, generator=g) * 3 - 1.5
    e.view(-1)[n // 3] = 1.75  # amax * s = 448 exactly
    out["amax_448"] = e
    return {k: v.to(dtype).contiguous() for k, v in out.items()}


QSHAPES = [(1, 128), (200, 256), (129, 768), (5, 131)]  # the last: a tail that is no multiple of 8 elements


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", QSHAPES, ids=[f"{m}x{k}" for m, k in QSHAPES])
def test_quantiser_matches_cpu_bitwise(cuda, shape, dtype):
    ins = _quant_inputs(shape, dtype)
    want = {k: F.quant_e4m3(v) for k, v in ins.items()}
    if shape[1] % 128 == 0:  # the constructions hit what they are meant to hit
        assert want["ties"].scale.item() == 1.0 and want["amax_448"].scale.item() == 256.0
        assert want["amax_pow2"].scale.item() == 64.0 and want["zero"].scale.item() == 1.0
        sr = want["subnormal_range"].q & 0x7f
        assert int(((sr > 0) & (sr < 8)).sum()) > shape[0] * shape[1] // 4
    dev = {k: v.cuda() for k, v in ins.items()}
    got = {k: F.quant_e4m3(v) for k, v in dev.items()}
    batch = F.quant_e4m3_batch(list(dev.values()))
    torch.cuda.synchronize()
    for (k, w), b in zip(want.items(), batch):
        for o, form in ((got[k], "single"), (b, "batched")):
            diff = int((o.q.cpu() != w.q).sum())
            print(f"FP8-QUANT | {shape} {dtype} {k} {form} | bytes differing {diff} | scale {o.scale.item():g}")
            assert diff == 0, f"{k} ({form}): {diff} of {w.q.numel()} bytes differ from the CPU path"
            assert torch.equal(o.scale.cpu().view(torch.int32), w.scale.view(torch.int32)), (k, form)
            assert torch.equal(o.inv.cpu().view(torch.int32), w.inv.view(torch.int32)), (k, form)


@gpu
def test_quantiser_batch_over_task_table_limit_and_preallocated(cuda):
    """More tensors than one task table holds (two launches), into preallocated outputs."""
    n = F.QT_MAX + 3
    xs = [(_r(3 + i % 5, 128, scale=1.0 + i, seed=i)).to(torch.bfloat16).cuda() for i in range(n)]
    qs = [torch.full(x.shape, 0xAA, dtype=torch.uint8, device="cuda") for x in xs]
    st = F.new_state(n, "cuda")
    out = F.quant_e4m3_batch(xs, qs, st)
    for x, o, q in zip(xs, out, qs):
        w = F.quant_e4m3(x.cpu())
        assert o.q is q and torch.equal(o.q.cpu(), w.q) and torch.equal(o.scale.cpu(), w.scale)
        assert torch.equal(o.inv.cpu(), w.inv)


# ------------------------------------------------------------------------------------------------ B1: exact

def _ints(M, Nn, K):
    i, j, k = torch.arange(M)[:, None], torch.arange(Nn)[:, None], torch.arange(K)[None, :]
    return ((7 * i + 3 * k) % 17 - 8).float(), ((5 * j + 11 * k) % 13 - 6).float()


def _as_fp8(v, inv=1.0):
    q = v.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), v)  # e4m3 holds these exactly
    return F.Fp8Tensor(q.view(torch.uint8).cuda(), torch.tensor([1.0 / inv]).cuda(), torch.tensor([inv]).cuda())


B1 = [(M, Nn, K, V64) for K in (128, 256, 768) for M in (1, 129, 200) for Nn in (16, 176, 400)]
B1 += [(2100, 2064, 256, V128), (129, 400, 256, "forced128")]


@gpu
@pytest.mark.parametrize("M,Nn,K,variant", B1, ids=[f"{m}x{n}x{k}-{v}" for m, n, k, v in B1])
def test_gemm_exact_integers(cuda, M, Nn, K, variant):
    a, b = _ints(M, Nn, K)
    want = (a.double() @ b.double().t()).float()
    forced = variant == "forced128"
    if forced:  # the 128-row tiles on a shape with ragged edges in both directions
        F.set_tile_m(128)
        variant = V128
    try:
        y = F.linear_fp8(_as_fp8(a), _as_fp8(b), None, out_dtype=torch.float32)
        _ran(variant, "bias", True, "exact integers")
        assert torch.equal(y.cpu(), want), f"{int((y.cpu() != want).sum())} of {want.numel()} elements differ"
        # the operands' scales: distinct powers of two, so a swapped or dropped one shows
        y = F.linear_fp8(_as_fp8(a, 2.0 ** -3), _as_fp8(b, 2.0 ** 5), None, out_dtype=torch.float32)
        _ran(variant, "bias", True, "exact integers, scaled")
        assert torch.equal(y.cpu(), want * 4.0)
    finally:
        if forced:
            F.set_tile_m(0)


@gpu
def test_gemm_refuses_unsupported_shapes(cuda):
    q = lambda r, c: F.Fp8Tensor(torch.zeros(r, c, dtype=torch.uint8, device="cuda"), torch.ones(1, device="cuda"),
                                 torch.ones(1, device="cuda"))
    for M, Nn, K in [(4, 32, 64), (4, 24, 128), (4, 32, 192)]:
        with pytest.raises(NotImplementedError):
            F.linear_fp8(q(M, K), q(Nn, K))


# ------------------------------------------------------------------------------------------------ B2: floor

B2 = [(200, 176, 128, V64), (129, 400, 256, V64), (256, 256, 768, V64), (300, 528, 3072, V64), (1, 176, 768, V64),
      (2100, 2064, 128, V128)]
DOMAIN = [0.0, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]


@gpu
@pytest.mark.parametrize("M,Nn,K,variant", B2, ids=[f"{m}x{n}x{k}-{v}" for m, n, k, v in B2])
def test_gemm_floor(cuda, M, Nn, K, variant):
    xq = F.quant_e4m3(_r(M, K, seed=100).to(torch.bfloat16))
    wq = F.quant_e4m3(_r(Nn, K, scale=0.05, seed=101).to(torch.bfloat16))
    a64, b64 = F.dequant(xq).double(), F.dequant(wq).double()
    acc, d = a64 @ b64.t(), a64.abs() @ b64.abs().t()
    fl = _floor(a64[:96], b64[:80])
    t = MARGIN * fl
    b = _r(Nn, seed=102).cuda()
    b64_ = b.double().cpu()
    res = _r(M, Nn, seed=103).cuda()
    r64 = res.double().cpu()
    xg, wg = _cuda(xq), _cuda(wq)
    tag = f"{variant} {M}x{Nn}x{K}"

    y = F.linear_fp8(xg, wg, None, out_dtype=torch.float32)
    _ran(variant, "bias", True, tag)
    _check(y, acc, _bound_f32(acc, d, t), tag + " f32 nobias", d, fl)
    y = F.linear_fp8(xg, wg, b, out_dtype=torch.float32)
    _ran(variant, "bias", True, tag)
    _check(y, acc + b64_, _bound_f32(acc + b64_, d, t, b64_.expand_as(acc)), tag + " f32", d, fl)
    y = F.linear_fp8(xg, wg, b)
    _ran(variant, "bias", False, tag)
    _check(y, acc + b64_, _bound_bf16(acc + b64_, d, t), tag + " bf16")
    for alias in (False, True):
        r = res.clone()
        y = F.linear_resid_fp8(xg, wg, b, r, out=r if alias else None)
        _ran(variant, "bias_resid", True, tag)
        ref = acc + b64_ + r64
        _check(y, ref, _bound_f32(ref, d, t, b64_.expand_as(acc), r64), tag + (" resid alias" if alias else " resid"), d, fl)
    for name, bias in (("gelu", b), ("gelu_domain", torch.tensor(DOMAIN).repeat((Nn + 8) // 9)[:Nn].contiguous().cuda())):
        u = acc + bias.double().cpu()
        g64, d64, dd64 = _gelu64(u)
        dk, gk = F.linear_gelu_fp8(xg, wg, bias)
        _ran(variant, "gelu_pair", False, tag)
        extra = EPS_EXP * (1 + u.abs())
        _check(gk, g64, _bound_bf16(g64, d, t, d64, extra), f"{tag} {name} g")
        _check(dk, d64, _bound_bf16(d64, d, t, dd64, extra), f"{tag} {name} d")
