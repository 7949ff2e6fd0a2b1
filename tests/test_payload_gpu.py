"""``csrc/payload.hip`` bit for bit: the bf16 DP gradient exchange's ``shard_sum_bf16`` and ``cast_bf16_to_f32``
(docs/NUMERICS.md, "Collectives").

Both kernels only add and convert.  ``shard_sum_bf16`` is the shard-ordered fp32 sum ``a = 0; a += float(x[j])``
rounded once to bf16; the cast is exact.  The emulations are plain torch on the CPU, written from the kernel
header and from no kernel output.  Every output sits between guard sentinels.  The unmarked tests need no GPU.
"""

import functools

import pytest
import torch

from distributed_training_compare_jax_amd.ops.payload import cast_bf16_to_f32, shard_sum_bf16

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD = 64               # elements: 128 bytes of bf16, 256 of fp32, so the guarded slice stays 16-byte aligned
CAP = 8 * (4096 * 256 + 3)   # three vector elements past one pass of the capped 4096 x 256 grid
SIZES = (8, 8 * 131, CAP)


@functools.lru_cache(maxsize=None)
def _shards(nshards, s):
    """bf16 [nshards, s], randn * 10^U(-2, 2)."""
    g = torch.Generator().manual_seed(1000 * nshards + s % 997)
    return (torch.randn(nshards, s, generator=g) * torch.pow(10.0, torch.rand(nshards, s, generator=g) * 4 - 2)).to(BF16)


def emu_shard_sum(x):
    a = torch.zeros(x.shape[1], dtype=torch.float32)
    for j in range(x.shape[0]):
        a = a + x[j].float()
    return a.to(BF16)


@functools.lru_cache(maxsize=None)
def _patterns(n):
    """Every bf16 bit pattern in order (finite values, +-0, +-inf, denormals, NaNs), tiled to n elements, and the
    fp32 bit pattern of each: the same 16 bits followed by 16 zero bits."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).repeat(-(-n // 65536))[:n].clone()
    return bits.view(BF16), bits.to(torch.int32) << 16


def _same_bits_bf16(got, exp):
    return torch.equal(got.view(torch.int16), exp.view(torch.int16))


def _guard(n, dtype, dev):
    buf = torch.full((n + 2 * GUARD,), 768.0, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == 768.0).all()) and bool((buf[GUARD + n:] == 768.0).all())


CASES = [(ns, s) for ns in (1, 2, 3, 8) for s in SIZES[:2]] + [(2, CAP)]


@gpu
@pytest.mark.parametrize("nshards,s", CASES)
def test_shard_sum_bf16_bitwise(cuda, nshards, s):
    x = _shards(nshards, s)
    exp = emu_shard_sum(x)
    buf, out = _guard(s, BF16, cuda)
    assert shard_sum_bf16(x.to(cuda).view(-1), nshards, out) is out
    assert _same_bits_bf16(out.cpu(), exp)
    assert _guards_intact(buf, s)
    cpu = torch.empty(s, dtype=BF16)
    shard_sum_bf16(x.view(-1), nshards, cpu)          # the torch branch of the gloo path: the same bits
    assert _same_bits_bf16(cpu, out.cpu())


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_cast_bf16_to_f32_bitwise_on_every_pattern(cuda, n):
    src, exp_bits = _patterns(n)
    nan = src.float().isnan()
    assert n < 65536 or int(nan.sum()) >= 254         # the full sweep holds every NaN pattern as well
    buf, dst = _guard(n, torch.float32, cuda)
    assert cast_bf16_to_f32(src.to(cuda), dst) is dst
    got = dst.cpu()
    assert torch.equal(got.view(torch.int32)[~nan], exp_bits[~nan])   # +-0, +-inf, denormals, every finite value
    assert bool(got[nan].isnan().all())
    assert _guards_intact(buf, n)
    cpu = torch.empty(n, dtype=torch.float32)
    cast_bf16_to_f32(src, cpu)
    assert torch.equal(cpu.view(torch.int32)[~nan], got.view(torch.int32)[~nan])


@gpu
def test_payload_kernels_refuse_partial_vectors(cuda):
    x = torch.zeros(24, dtype=BF16, device=cuda)
    out = torch.full((12,), 768.0, dtype=BF16, device=cuda)
    with pytest.raises(RuntimeError):
        shard_sum_bf16(x, 2, out)                      # s = 12
    dst = torch.full((12,), 768.0, device=cuda)
    with pytest.raises(RuntimeError):
        cast_bf16_to_f32(x[:12], dst)                  # n = 12
    torch.cuda.synchronize()
    assert bool((out == 768.0).all()) and bool((dst == 768.0).all())


# ------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("nshards,s", [(ns, s) for ns in (1, 2, 3, 8) for s in SIZES[:2]])
def test_shard_sum_torch_branch_is_the_shard_ordered_sum(nshards, s):
    """The CPU branch (``.float().sum(0)``) against the explicit loop: the same bits, so the gloo path and the
    kernel agree with one another through the emulation."""
    x = _shards(nshards, s)
    out = torch.empty(s, dtype=BF16)
    shard_sum_bf16(x.view(-1), nshards, out)
    assert _same_bits_bf16(out, emu_shard_sum(x))


def test_cast_torch_branch_is_exact_on_every_pattern():
    src, exp_bits = _patterns(65536)
    nan = src.float().isnan()
    dst = torch.empty(65536, dtype=torch.float32)
    cast_bf16_to_f32(src, dst)
    assert torch.equal(dst.view(torch.int32)[~nan], exp_bits[~nan]) and bool(dst[nan].isnan().all())
    assert int(nan.sum()) == 254 and int(dst.isinf().sum()) == 2


@pytest.mark.parametrize("nshards", (2, 3, 8))
def test_selfcheck_shard_sum_comparison_rejects_wrong_sums(nshards):
    x = _shards(nshards, 8 * 131)
    exp = emu_shard_sum(x)
    ref = x.double().sum(0)
    mag = x.double().abs().sum(0)
    a = x.float().sum(0)
    half_ulp = torch.ldexp(torch.ones(a.numel(), dtype=torch.float64), torch.frexp(a)[1] - 9)
    assert bool(((exp.double() - ref).abs() <= half_ulp + nshards * 2.0 ** -24 * mag).all())
    assert not _same_bits_bf16(emu_shard_sum(x[:-1]), exp)                       # the last shard dropped
    acc = torch.zeros(8 * 131, dtype=BF16)                                       # a bf16 accumulator
    for j in range(nshards):
        acc = (acc.float() + x[j].float()).to(BF16)
    assert nshards == 2 or not _same_bits_bf16(acc, exp)
    trunc = (x.float().sum(0).view(torch.int32) & -65536).view(torch.float32).to(BF16)   # truncated, not rounded
    assert not _same_bits_bf16(trunc, exp)
