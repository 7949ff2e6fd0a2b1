"""``rope_`` on the GPU (``csrc/rope.hip``) per element against the float64 rotation and the derived bound of
tests/test_rope_cpu.py, forward and inverse; the entry point's refusals; a captured replay against the eager call."""

import pytest
import torch
from test_rope_cpu import amplitudes, bound, rotate64

from distributed_training_compare_jax_amd.ops.rope import rope_, rope_table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [1, 72, 130])  # B * T not a multiple of 4: a partly filled last block
@pytest.mark.parametrize("H,Hkv,hd", [(2, 2, 32), (4, 2, 64), (3, 1, 64), (6, 2, 128), (5, 5, 128)])
def test_rope_matches_float64(cuda, H, Hkv, hd, T, dtype):
    tab = rope_table(130, hd, 10000.0, cuda)
    x, n = amplitudes((2, T, (H + 2 * Hkv) * hd), dtype).to(cuda), (H + Hkv) * hd
    for inverse in (False, True):
        y = rope_(x.clone(), tab, H, Hkv, inverse=inverse)
        ref, mag = rotate64(x, tab, H + Hkv, inverse)
        assert ((y.double().cpu() - ref).abs() <= bound(ref, mag, dtype)).all(), f"inverse={inverse}"
        assert torch.equal(y[..., n:], x[..., n:]), "the V columns changed"
        assert torch.equal(y[:, 0], x[:, 0]), "position 0 (cos 1, sin 0) changed"
    # the round trip: twice the bound of x; in bf16 the relative term is of |lo| + |hi|, since the rounding of the
    # rotated tensor in between returns into both elements of a pair whatever their own size (docs/NUMERICS.md)
    back = rope_(rope_(x.clone(), tab, H, Hkv), tab, H, Hkv, inverse=True).double().cpu()
    x64 = x.double().cpu()
    assert ((back - x64).abs() <= 2 * bound(mag if dtype == torch.bfloat16 else x64, mag, dtype)).all()


@pytest.mark.parametrize("case", ["heads", "head_dim", "table", "align"])
def test_refusals_leave_the_tensor_untouched(cuda, case):
    H, Hkv, hd, T = (3, 2, 64, 8) if case == "heads" else (2, 2, 48 if case == "head_dim" else 64, 8)
    tab = rope_table(4 if case == "table" else 16, hd, 10000.0, cuda)
    n = 2 * T * (H + 2 * Hkv) * hd
    buf = torch.randn(n + 8, device=cuda).to(torch.bfloat16)
    off = 1 if case == "align" else 0  # one bf16 element: 2 bytes off a 16-byte boundary
    keep = buf.clone()
    with pytest.raises((RuntimeError, ValueError)):
        rope_(buf[off:off + n].view(2, T, -1), tab, H, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


def test_second_run_and_graph_replay_repeat_the_first(cuda):
    H, Hkv, hd = 4, 2, 64
    tab = rope_table(130, hd, 10000.0, cuda)
    x = amplitudes((2, 72, (H + 2 * Hkv) * hd), torch.bfloat16, seed=1).to(cuda)
    first, buf = rope_(x.clone(), tab, H, Hkv), x.clone()
    assert torch.equal(rope_(x.clone(), tab, H, Hkv), first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rope_(buf, tab, H, Hkv)
    for _ in range(3):
        buf.copy_(x)
        graph.replay()
        assert torch.equal(buf, first)
