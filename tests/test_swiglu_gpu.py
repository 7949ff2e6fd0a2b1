"""The SwiGLU kernels (``csrc/swiglu.hip`` through ``ops/swiglu.py``) per element against float64 from the same bf16 / fp32
inputs (docs/NUMERICS.md, "SwiGLU").  ``D = |A| . |B|``, ``T(K)`` the componentwise tolerance of a K-long fp32 dot product
(the helper of tests/test_gemm_floor_gpu.py, copied), ``s = sigmoid(g)``, ``silu = g s``, ``silu' = s (1 + g (1 - s))``:

    gu    2^-8 |ref| + T(K) D
    h     2^-8 |ref| + |silu'(g)| |u| T(K) D_g + |silu(g)| T(K) D_u + 2^-20 (1 + |g|) |u|
    dgu   2^-8 |ref| + T(K) D_dh |factor| + 2^-20 (1 + |g|) |other|      factor = u silu'(g) | silu(g), other = dh u | dh

The elementwise kernels alone have no dot product: ``eps |ref|`` + the last term, ``eps`` = 2^-8 (bf16 out) or 2^-22 (fp32).
The gate bias runs from -30 to 30, so both saturated tails of the sigmoid are in every case."""

import functools

import pytest
import torch

from distributed_training_compare_jax_amd.ops import swiglu as SW

pytestmark = pytest.mark.gpu

EPS_BF16, EPS_F32, EPS_EXP = 2.0 ** -8, 2.0 ** -22, 2.0 ** -20
# (M, D, F): one tile and one k-step; fewer rows than a wave tile; ragged rows, odd k-step count, 5 hidden tiles (an odd
# count for the backward's 128-wide tiles); one row past a tile and many hidden tiles; a GPT-2-small-like K
SHAPES = [(128, 64, 64), (4, 64, 64), (200, 192, 320), (257, 128, 1088), (130, 768, 2048)]


def _r(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + 0.1 * torch.rand(*shape, generator=g)


def _trunc32(x64):
    y = x64.float()
    return torch.where(y.double().abs() > x64.abs(), torch.nextafter(y, torch.zeros_like(y)), y).double()


@functools.lru_cache(maxsize=None)
def T(K):
    """4x the worst error / D of a pessimistic fp32 accumulation (blocks of 8 exact products, the running sum truncated
    toward zero) on a 96 x 80 sub-problem of the generators."""
    a, b = _r(96, K, seed=9001).bfloat16().double(), _r(80, K, scale=0.05, seed=9002).bfloat16().double()
    acc = torch.zeros(96, 80, dtype=torch.float64)
    for k0 in range(0, K, 8):
        acc = _trunc32(acc + a[:, k0:k0 + 8] @ b[:, k0:k0 + 8].t())
    return 4.0 * ((acc - a @ b.t()).abs() / (a.abs() @ b.abs().t())).max().item()


def _gate(g):
    s = torch.sigmoid(g)
    return g * s, s * (1 + g * (1 - s))  # silu, silu'


def _check(out, ref, bound, name):
    o = out.double().cpu()
    ratio = ((o - ref).abs() / (bound + 1e-30)).max().item()
    print(f"SWIGLU | {name} | err/bound {ratio:.3f}")
    assert bool(torch.isfinite(o).all()) and ratio <= 1.0, (name, ratio)


@functools.lru_cache(maxsize=None)
def _case(M, D, F):
    """bf16 inputs on the GPU and the float64 references with their bounds, built once per shape."""
    x, w = _r(M, D, seed=1).bfloat16(), _r(2 * F, D, scale=0.05, seed=2).bfloat16()
    b = torch.cat([torch.linspace(-30, 30, F), _r(F, seed=3)])
    dy, w2 = _r(M, D, seed=4).bfloat16(), _r(D, F, scale=0.05, seed=5).bfloat16()
    gu_in = (_r(M, 2 * F, seed=6) + b).bfloat16()  # the backward's saved pre-activations, |g| to about 30
    t = T(D)
    gu = x.double() @ w.double().t() + b.double()
    dgu_d = t * (x.double().abs() @ w.double().abs().t())
    (g, u), (dg_, du_) = gu.split(F, 1), dgu_d.split(F, 1)
    silu, dsilu = _gate(g)
    fwd = dict(gu=(gu, EPS_BF16 * gu.abs() + dgu_d),
               h=(silu * u, EPS_BF16 * (silu * u).abs() + dsilu.abs() * u.abs() * dg_ + silu.abs() * du_
                  + EPS_EXP * (1 + g.abs()) * u.abs()))
    dh, ddh = dy.double() @ w2.double(), t * (dy.double().abs() @ w2.double().abs())
    g, u = gu_in.double().split(F, 1)
    silu, dsilu = _gate(g)
    ref = torch.cat([dh * u * dsilu, dh * silu], 1)
    fac, oth = torch.cat([u * dsilu, silu], 1).abs(), torch.cat([dh * u, dh], 1).abs()
    bwd = (ref, EPS_BF16 * ref.abs() + torch.cat([ddh, ddh], 1) * fac + EPS_EXP * (1 + torch.cat([g, g], 1).abs()) * oth)
    dev = [v.cuda() for v in (x, w, b, dy, w2, w2.t().contiguous(), gu_in)]
    return dev, fwd, bwd


def _run(M, D, F, want, tag):
    (x, w, b, dy, w2, w2t, gu_in), fwd, bwd = _case(M, D, F)
    gu, h = SW.swiglu_fc1(x, w, b)
    assert SW.LAST["fc1"] == want
    dgu = SW.swiglu_fc2_dgrad(dy, w2, w2t, gu_in)
    assert SW.LAST["fc2_dgrad"] == want
    for name, out, (ref, bound) in (("gu", gu, fwd["gu"]), ("h", h, fwd["h"]), ("dgu", dgu, bwd)):
        _check(out, ref, bound, f"{tag} {M}x{D}x{F} {name}")
    return gu, h, dgu


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_pair_vs_float64(cuda, shape):
    a = _run(*shape, "fused", "fused")
    if shape == SHAPES[2]:  # no atomics, a fixed summation order: a second run gives the same bits
        assert all(torch.equal(p, q) for p, q in zip(a, _run(*shape, "fused", "fused again")))


@pytest.mark.parametrize("shape,knob", [((130, 64, 96), "1"), (SHAPES[2], "0")], ids=["F_not_a_tile_multiple", "knob_off"])
def test_unfused_path_same_bounds(cuda, monkeypatch, shape, knob):
    """F % 64 != 0, or ``DTC_SWIGLU_FUSE=0``: the ordinary GEMMs (fp32 out) + the elementwise kernels, recorded ``unfused``,
    within the fused pair's bounds.  ``gu`` of the two paths is NOT asserted bitwise equal: the kernels place k
    differently inside an MFMA, whose internal summation order is undocumented."""
    monkeypatch.setenv("DTC_SWIGLU_FUSE", knob)
    _run(*shape, "unfused", "unfused")
    (x, w, b, dy, w2, _, gu_in), _, bwd = _case(*shape)
    dgu = SW.swiglu_fc2_dgrad(dy, w2, None, gu_in)  # no transposed mirror: the NN dgrad in front
    assert SW.LAST["fc2_dgrad"] == "unfused"
    _check(dgu, *bwd, "unfused, no mirror, dgu")


@pytest.mark.parametrize("src,dst", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32),
                                     (torch.float32, torch.bfloat16)], ids=["bf16", "fp32", "fp32_to_bf16"])
def test_elementwise_kernels_vs_float64(cuda, src, dst):
    M, F = 37, 100  # not a multiple of a block, rows of 25 four-element groups
    gu = (_r(M, 2 * F, seed=7) + torch.cat([torch.linspace(-30, 30, F), torch.zeros(F)])).to(src)
    dh = _r(M, F, seed=8)
    g, u = gu.double().split(F, 1)
    silu, dsilu = _gate(g)
    eps = EPS_F32 if dst == torch.float32 else EPS_BF16
    gu_o, h = SW.swiglu_act(gu.cuda(), dst)
    assert gu_o.dtype == dst and torch.equal(gu_o.cpu(), gu.to(dst))
    _check(h, silu * u, eps * (silu * u).abs() + EPS_EXP * (1 + g.abs()) * u.abs(), f"act {src}->{dst}")
    if src == dst:
        ref = torch.cat([dh.double() * u * dsilu, dh.double() * silu], 1)
        oth = torch.cat([dh.double() * u, dh.double()], 1).abs()
        _check(SW.swiglu_act_bwd(dh.cuda(), gu.cuda()), ref,
               eps * ref.abs() + EPS_EXP * (1 + torch.cat([g, g], 1).abs()) * oth, f"act bwd {src}")
