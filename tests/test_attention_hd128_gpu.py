"""head_dim 128 causal flash attention, bf16 (csrc/attention.hip: attn_fwd32<128>, attn_bwd_dkdv32<128>,
attn_bwd_dq32<128>) and exact fp32 (csrc/attention_f32.hip at HD = 128), against the float64 materialised softmax.

bf16 uses the project's scale-aware metric (docs/NUMERICS.md, tests/test_kernels_scale_gpu.py): per (batch, head,
16 rows) at 2e-2 (o) / 3e-2 (dQ, dK, dV) of the block's own maximum, lse to 1e-3 absolute.  The float64 emulation
of a correct bf16 kernel's rounding (``_attn_emulate``) alone gives these worst-block errors (CPU):

    shape                 o        dQ       dK       dV
    (1,1024,2,128)        5.6e-3   5.9e-3   4.9e-3   4.7e-3
    (1,1024,2,128) spike  4.9e-3   1.0e-1   1.1e-2   4.9e-3
    (1,777,3,128)         4.7e-3   5.4e-3   5.1e-3   4.7e-3
    (2,200,2,128)         4.9e-3   5.6e-3   5.8e-3   5.0e-3
    (1,72,1,128)          4.3e-3   4.4e-3   5.7e-3   4.3e-3

so every asserted tensor has at least 2.7x headroom; the tests assert that floor too (< 1e-2 on the non-spike
shapes).  Spike dQ is printed, not asserted: delta = rowsum(dO * O) from the bf16-rounded O leaves 1.0e-1 of the
block's maximum in the emulation of that rounding alone (the docs/NUMERICS.md finding).

fp32 uses the metric and tolerances of tests/test_kernels_f32_gpu.py::test_f32_flash_attention.

Shapes: one ragged tile (72), batch and head strides with T % 64 != 0 (200), odd T with three heads (777), eight
full 128-query blocks with diagonal and off-diagonal tiles (1024).
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

from test_kernels_f32_gpu import _close as _close_f32
from test_kernels_f32_gpu import _r as _r_f32
from test_kernels_gpu import _attn_ref64
from test_kernels_scale_gpu import BLOCK, _attn_case, _close_blocks, _report

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A

pytestmark = pytest.mark.gpu

SHAPES = [(1, 72, 1, 128), (2, 200, 2, 128), (1, 777, 3, 128), (1, 1024, 2, 128)]
CASES = [pytest.param(s, False, id="x".join(map(str, s))) for s in SHAPES] + [
    pytest.param(SHAPES[3], True, id="1x1024x2x128-spike")]
FWD, BWD = "attn_fwd32<128>", "attn_bwd_{dkdv32,dq32}<128>"
# what A.last_launch() must name after a head_dim 128 call, whatever the flags
FWD_KERNELS = ("attn_fwd32_kernel<128>",)
BWD_KERNELS = ("attn_delta_kernel<128>", "attn_bwd_dkdv32_kernel<128>", "attn_bwd_dq32_kernel<128,true>")


@pytest.mark.parametrize("shape,spike", CASES)
def test_hd128_fwd_blocks(cuda, shape, spike):
    """Observed on the MI355X: see docs/NUMERICS.md (kernel / emulation ratios of the SCALE-RATIO lines)."""
    B, T, H, hd = shape
    qkv, _, ref, floor = _attn_case(B, T, H, hd, spike)
    o, lse = A.attn_fwd(qkv.to(cuda), H)
    assert A.last_launch().kernels == FWD_KERNELS, A.last_launch()
    assert o.dtype == torch.bfloat16 and lse.dtype == torch.float32 and lse.shape == (B, H, T)
    o = o.view(B, T, H, hd)
    _report(FWD, shape, spike, "o", o, ref, floor)
    lse_err = (lse.cpu().double() - ref["lse"]).abs().max().item()
    print(f"SCALE-LSE | {FWD} | {shape}{' spike' if spike else ''} | max abs err {lse_err:.3e}")
    assert floor["o"] < 1e-2, floor
    _close_blocks(o, ref["o"], 2e-2, BLOCK, 1, "o")
    assert lse_err <= 1e-3, f"lse: max abs err {lse_err:.3e} > 1e-3"


@pytest.mark.parametrize("shape,spike", CASES)
def test_hd128_bwd_blocks(cuda, shape, spike):
    """The backward gets the GPU forward's own o and lse, as in training; the reference is independent of both."""
    B, T, H, hd = shape
    qkv, do, ref, floor = _attn_case(B, T, H, hd, spike)
    qkv_d, do_d = qkv.to(cuda), do.to(cuda)
    o, lse = A.attn_fwd(qkv_d, H)
    d = A.attn_bwd(qkv_d, o, lse, do_d, H).view(B, T, 3, H, hd)
    assert A.last_launch().kernels == BWD_KERNELS, A.last_launch()
    outs = {n: d[:, :, "qkv".index(n[1])] for n in ("dq", "dk", "dv")}
    for n, t in outs.items():
        _report(BWD, shape, spike, n, t, ref, floor)
    asserted = ("dk", "dv") if spike else ("dq", "dk", "dv")
    if not spike:
        assert max(floor[n] for n in asserted) < 1e-2, floor
    for n in asserted:
        _close_blocks(outs[n], ref[n], 3e-2, BLOCK, 1, n)


@functools.lru_cache(maxsize=None)
def _f32_case(B, T, H, hd):
    qkv, do = _r_f32(B, T, 3 * H * hd, seed=16), _r_f32(B, T, H * hd, seed=17)
    return (qkv, do) + _attn_ref64(qkv, do, H)


@pytest.mark.parametrize("shape", [pytest.param(s, id="x".join(map(str, s))) for s in SHAPES])
def test_hd128_f32(cuda, shape):
    B, T, H, hd = shape
    qkv, do, oref, lseref, dref = _f32_case(B, T, H, hd)
    o, lse = A.attn_fwd(qkv.to(cuda), H)
    assert o.dtype == torch.float32
    _close_f32(o, oref, 1e-5, "o")
    _close_f32(lse, lseref, 1e-6, "lse")
    dqkv = A.attn_bwd(qkv.to(cuda), o, lse, do.to(cuda), H).view(B, T, 3, H, hd)
    dref = dref.view(B, T, 3, H, hd)
    for i, name in enumerate(("dq", "dk", "dv")):
        _close_f32(dqkv[:, :, i], dref[:, :, i], 1e-5, name)


def _inputs(shape, dtype, cuda):
    B, T, H, hd = shape
    if dtype == torch.bfloat16:
        qkv, do, _, _ = _attn_case(B, T, H, hd)
    else:
        qkv, do = _f32_case(B, T, H, hd)[:2]
    return qkv.to(cuda), do.to(cuda)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_hd128_deterministic(cuda, dtype):
    """No atomics anywhere: two calls of the forward and of the backward return identical bits."""
    H = SHAPES[2][2]
    qkv, do = _inputs(SHAPES[2], dtype, cuda)
    o1, l1 = A.attn_fwd(qkv, H)
    o2, l2 = A.attn_fwd(qkv, H)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    d1 = A.attn_bwd(qkv, o1, l1, do, H)
    d2 = A.attn_bwd(qkv, o1, l1, do, H)
    assert torch.equal(d1, d2)
    assert bool(torch.isfinite(d1.float()).all())
    if dtype == torch.bfloat16:  # head_dim 128 ignores every flag: same record, same bits
        bwd = A.last_launch()
        assert torch.equal(d1, A.attn_bwd(qkv, o1, l1, do, H, flags=15)) and A.last_launch() == bwd
        assert bwd.kernels == BWD_KERNELS, bwd
        o3, l3 = A.attn_fwd(qkv, H)
        fwd = A.last_launch()
        o4, l4 = A.attn_fwd(qkv, H, flags=127)
        assert A.last_launch() == fwd and fwd.kernels == FWD_KERNELS, (fwd, A.last_launch())
        assert torch.equal(o3, o4) and torch.equal(l3, l4) and torch.equal(o3, o1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_hd128_batch_slice_bitwise(cuda, dtype):
    """Batch element 0 of the B = 2 call equals a B = 1 call on its slice, bitwise: nothing of another (b, h)
    leaks through the LDS stages or the ragged last tile."""
    H = SHAPES[1][2]
    qkv, do = _inputs(SHAPES[1], dtype, cuda)
    o, lse = A.attn_fwd(qkv, H)
    d = A.attn_bwd(qkv, o, lse, do, H)
    q0, do0 = qkv[:1].contiguous(), do[:1].contiguous()
    o0, lse0 = A.attn_fwd(q0, H)
    assert torch.equal(o0, o[:1]) and torch.equal(lse0, lse[:1])
    d0 = A.attn_bwd(q0, o0, lse0, do0, H)
    assert torch.equal(d0, d[:1])


def test_unsupported_head_dim_still_raises(cuda, monkeypatch):
    """head_dim 96: NotImplementedError naming 32/64/128, raised before the library is touched."""
    def no_launch():
        raise AssertionError("the kernel library was reached")

    qkv = torch.zeros(1, 64, 3 * 2 * 96, dtype=torch.bfloat16, device=cuda)
    monkeypatch.setattr(N, "lib", no_launch)
    with pytest.raises(NotImplementedError, match="32/64/128"):
        A.attn_fwd(qkv, 2)


DEBUG_SCRIPT = r"""
import sys
import torch
from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A

B, T, H, hd = 2, 200, 2, 128
g = torch.Generator().manual_seed(7)
qkv = torch.randn(B, T, 3 * H * hd, generator=g)
do = torch.randn(B, T, H * hd, generator=g)
out = {}
for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
    q, d = qkv.to(dt).cuda(), do.to(dt).cuda()
    o, lse = A.attn_fwd(q, H)
    dqkv = A.attn_bwd(q, o, lse, d, H)
    torch.cuda.synchronize()
    out[name] = (o.float().cpu(), lse.cpu(), dqkv.float().cpu())
print("LIB", N.LIB_PATH)
torch.save(out, sys.argv[1])
"""


def test_hd128_debug_library_asserts_clean(cuda, tmp_path):
    """The -DDTC_DEBUG library (every DTC_ASSERT of the index math live) runs the head_dim 128 kernels of both
    precisions on a ragged two-batch shape without tripping an assert and agrees with the release library.
    Each library runs in its own child process, as in tests/test_debug_build_gpu.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "distributed_training_compare_jax_amd")
    outs = {}
    for tag, lib in (("debug", "_dtc_kernels_debug.so"), ("release", "_dtc_kernels.so")):
        lib = os.path.join(pkg, lib)
        assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() builds it in-tree"
        dst = str(tmp_path / f"{tag}.pt")
        r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT, dst], cwd=root, capture_output=True, text=True,
                           env=dict(os.environ, DTC_KERNEL_LIB=lib, PYTHONPATH=root), timeout=120)
        assert r.returncode == 0, f"{tag} library exited {r.returncode}:\n{(r.stdout + r.stderr)[-4000:]}"
        assert f"LIB {lib}" in r.stdout, r.stdout[-2000:]
        outs[tag] = torch.load(dst)
    for name, rtol in (("bf16", 2e-2), ("fp32", 1e-5)):  # -O1 may contract differently: not bitwise
        for a, b, what in zip(outs["debug"][name], outs["release"][name], ("o", "lse", "dqkv")):
            err, mag = (a - b).abs().max().item(), b.abs().max().item()
            assert err <= rtol * mag, f"{name} {what}: debug vs release {err:.3e} > {rtol:.0e} * {mag:.3e}"
