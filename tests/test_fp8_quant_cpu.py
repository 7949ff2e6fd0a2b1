"""The e4m3 quantiser's definition (the torch CPU path of ``ops/fp8.py``) and the CPU forms of the FP8 linears.

The GPU kernels are held to this path bit for bit in ``tests/test_fp8_gpu.py``; here its properties are checked:
the scale is a power of two, ``amax * s`` lies in (224, 448], zero gives ``s = 1``, representable values round-trip,
ties go to even."""

import math

import pytest
import torch

from distributed_training_compare_jax_amd.ops import fp8 as F
from distributed_training_compare_jax_amd.ops import gemm as G


def _is_pow2(v: float) -> bool:
    m, _ = math.frexp(v)
    return m == 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mag", [1e-30, 3e-7, 0.02, 1.0, 1.75, 1.7500001, 2.0, 447.0, 448.0, 449.0, 6e4, 3e30])
def test_scale_is_power_of_two_and_fills_the_range(dtype, mag):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 128, generator=g) * mag).to(dtype)
    t = F.quant_e4m3(x)
    s, inv = t.scale.item(), t.inv.item()
    amax = x.float().abs().max().item()
    assert t.q.dtype == torch.uint8 and tuple(t.q.shape) == (8, 128)
    assert t.scale.dtype == torch.float32 and t.inv.dtype == torch.float32
    assert _is_pow2(s) and _is_pow2(inv) and s * inv == 1.0
    assert 224.0 < amax * s <= 448.0, (amax, s)
    # one rounding of the exactly scaled value: at most half an e4m3 step (2^-4 relative) or half a subnormal step
    deq = F.dequant(t)
    err = (deq - x.float()).abs()
    assert bool((err <= torch.maximum(x.float().abs() * 2.0 ** -4, torch.tensor(2.0 ** -10 * inv))).all())


@pytest.mark.parametrize("amax,want_scaled", [(1.0, 256.0), (4.0, 256.0), (1.75, 448.0), (0.4375, 448.0),
                                              (1.875, 240.0), (2.0 ** -20, 256.0), (3.0 * 2.0 ** 60, 384.0)])
def test_scaled_amax(amax, want_scaled):
    x = torch.zeros(1, 128)
    x[0, 5] = -amax
    t = F.quant_e4m3(x)
    assert amax * t.scale.item() == want_scaled


def test_scale_exponent_is_clamped_to_normal_fp32():
    for amax in (1e-45, 2.0 ** -140, 2.0 ** -127):
        x = torch.zeros(1, 128)
        x[0, 0] = amax
        t = F.quant_e4m3(x)
        assert t.scale.item() == 2.0 ** 126 and t.inv.item() == 2.0 ** -126
    x = torch.zeros(1, 128)
    x[0, 0] = 3e38
    t = F.quant_e4m3(x)
    assert t.scale.item() == 2.0 ** -120 and 224 < 3e38 * t.scale.item() <= 448  # 3e38 = 1.763 * 2^127


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_tensor(dtype):
    t = F.quant_e4m3(torch.zeros(3, 128, dtype=dtype))
    assert t.scale.item() == 1.0 and t.inv.item() == 1.0
    assert int(t.q.count_nonzero()) == 0


def test_representable_values_round_trip():
    """Every finite e4m3 value, put at a scale where 448 is the amax: quantise(dequantise) is the identity."""
    codes = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    for k in (-9, 0, 5):
        x = torch.zeros(2, 128)
        x.view(-1)[:codes.numel()] = vals * 2.0 ** k
        t = F.quant_e4m3(x)
        assert t.scale.item() == 2.0 ** -k
        got = t.q.view(-1)[:codes.numel()]
        same = (got == codes) | ((codes & 0x7f) == 0)  # +-0: the byte keeps the sign of the product
        assert bool(same.all())
        assert torch.equal(F.dequant(t), x)


def test_ties_go_to_even():
    x = torch.zeros(1, 128)
    x[0, 0] = 256.0  # amax: s = 1
    ties = [17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 34.0, 38.0, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 0.5 * 2.0 ** -9,
            7.5 * 2.0 ** -9]
    want = [16.0, 20.0, 20.0, 24.0, -16.0, -20.0, 32.0, 40.0, 2.0 * 2.0 ** -9, 2.0 * 2.0 ** -9, 0.0, 2.0 ** -6]
    x[0, 1:1 + len(ties)] = torch.tensor(ties)
    t = F.quant_e4m3(x)
    assert t.scale.item() == 1.0
    assert F.dequant(t)[0, 1:1 + len(ties)].tolist() == want


def test_batch_equals_single_and_fills_preallocated_outputs():
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(4, 128, generator=g), (torch.randn(3, 256, generator=g) * 50).to(torch.bfloat16),
          torch.zeros(2, 128)]
    single = [F.quant_e4m3(x) for x in xs]
    batch = F.quant_e4m3_batch(xs)
    qs = [torch.empty(x.shape, dtype=torch.uint8) for x in xs]
    st = F.new_state(len(xs), "cpu")
    pre = F.quant_e4m3_batch(xs, qs, st)
    for s, b, p, q in zip(single, batch, pre, qs):
        for o in (b, p):
            assert torch.equal(s.q, o.q) and torch.equal(s.scale, o.scale) and torch.equal(s.inv, o.inv)
        assert p.q is q


def test_rejects_other_dtypes_and_layouts():
    with pytest.raises(TypeError):
        F.quant_e4m3(torch.zeros(2, 128, dtype=torch.float16))
    with pytest.raises(ValueError):
        F.quant_e4m3(torch.zeros(128, 4).t())
    with pytest.raises(ValueError):
        F.quant_e4m3(torch.zeros(128))


# ------------------------------------------------------------------------------------------- CPU linears

def _ops(M=5, Nn=32, K=128, seed=3):
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) * 0.05
    return F.quant_e4m3(x), F.quant_e4m3(w), torch.randn(Nn, generator=g)


def test_cpu_linears_compute_on_the_dequantised_operands():
    xq, wq, b = _ops()
    u = F.dequant(xq) @ F.dequant(wq).t() + b
    assert torch.equal(F.linear_fp8(xq, wq, b, out_dtype=torch.float32), u)
    assert F.linear_fp8(xq, wq, b).dtype == torch.bfloat16
    r = torch.randn(5, 32, generator=torch.Generator().manual_seed(4))
    out = r.clone()
    assert F.linear_resid_fp8(xq, wq, b, out, out=out) is out and torch.equal(out, u + r)
    d, gl = F.linear_gelu_fp8(xq, wq, b, out_dtype=torch.float32)
    assert torch.equal(d, G.gelu_tanh_grad(u)) and torch.equal(gl, G.gelu_tanh(u))


@pytest.mark.parametrize("M,Nn,K", [(4, 32, 64), (4, 24, 128), (4, 32, 192)])
def test_unsupported_shapes_raise_before_any_launch(M, Nn, K):
    q = lambda r, c: F.Fp8Tensor(torch.zeros(r, c, dtype=torch.uint8), torch.ones(1), torch.ones(1))
    for fn in (lambda: F.linear_fp8(q(M, K), q(Nn, K)), lambda: F.linear_resid_fp8(q(M, K), q(Nn, K), None, None),
               lambda: F.linear_gelu_fp8(q(M, K), q(Nn, K), None)):
        with pytest.raises(NotImplementedError):
            fn()
