"""Grouped-query attention kernels (csrc/attention.hip).  Bit for bit against the 32-row multi-head kernels on repeated
K/V heads (``ROUND4`` / ``FORCE_MERGED`` pick that family at head_dim 64) where the arithmetic is theirs: o, lse, dQ,
and with Hkv == H (through the GQA entry points: the ops route that to the multi-head path) dK / dV too.  dK / dV, the
group sums, against float64 at the bound docs/NUMERICS.md fixes for the 32-row backward (3e-2 of a 16-row block's
maximum); dO of every group's first query head is 16x the others', so a lost head or another head's lse / delta misses
by orders of magnitude.  (8, 2) fills one whole run of gqa_block's transposed order at G = 4."""

import pytest
import torch

from test_kernels_scale_gpu import BLOCK, _close_blocks
from test_kernels_gpu import _r

from distributed_training_compare_jax_amd.ops import _native as N
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.ops.gemm import _workspace

pytestmark = pytest.mark.gpu
B = 2
CASES = ([(4, 4, hd, T) for hd in (64, 128) for T in (200, 328)] + [(8, 2, 64, 200), (8, 2, 128, 200)]
         + [(H, Hkv, hd, T) for H, Hkv in ((4, 2), (4, 1), (6, 2)) for hd in (64, 128) for T in (72, 200, 328)])
BWD = {64: ("bwd_rows32_gqa_merged", ("attn_delta_kernel<64>", "attn_bwd_merged32_gqa_kernel<64>")),
       128: ("bwd_rows32_gqa_128", ("attn_delta_kernel<128>", "attn_bwd_dkdv32_gqa_kernel<128>",
                                    "attn_bwd_dq32_gqa_kernel<128>"))}


def ref64(qkv, do, H, Hkv, hd):
    """float64 dK, dV [B, T, Hkv, hd] by autograd through repeated K/V heads."""
    T = qkv.shape[1]
    q, k, v = (t.clone().requires_grad_(True) for t in qkv.cpu().double().split([H * hd, Hkv * hd, Hkv * hd], -1))
    kr, vr = (t.view(B, T, Hkv, hd).repeat_interleave(H // Hkv, 2) for t in (k, v))
    s = torch.einsum("bthd,bshd->bhts", q.view(B, T, H, hd), kr) * hd ** -0.5
    s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), vr).backward(do.cpu().double().view(B, T, H, hd))
    return k.grad.view(B, T, Hkv, hd), v.grad.view(B, T, Hkv, hd)


@pytest.mark.parametrize("H,Hkv,hd,T", CASES)
def test_against_multi_head_and_float64(cuda, H, Hkv, hd, T):
    qkv, do, nqb, w = _r(B, T, (H + 2 * Hkv) * hd, seed=30), _r(B, T, H, hd, seed=31), -(-T // 128), [H * hd, Hkv * hd, Hkv * hd]
    do[:, :, ::H // Hkv] *= 16
    do = do.view(B, T, H * hd)
    if Hkv < H:
        o, lse = A.attn_fwd(qkv, H, n_kv_heads=Hkv)
        fwd = A.last_launch()
        dqkv = A.attn_bwd(qkv, o, lse, do, H, n_kv_heads=Hkv)
        assert A.plan_fwd(B, T, H, hd, n_kv_heads=Hkv) == fwd and A.plan_bwd(B, T, H, hd, n_kv_heads=Hkv) == A.last_launch()
    else:
        L, st, ws = N.lib(), N.stream_ptr(cuda), _workspace(cuda, 4 * B * H * T)
        o, lse, dqkv = torch.empty_like(do), torch.empty(B, H, T, device=cuda), torch.empty_like(qkv)
        N.check(L.dtc_attn_fwd_gqa(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, T, H, Hkv, hd, 0, hd ** -0.5, st), "fwd")
        fwd = A.last_launch()
        N.check(L.dtc_attn_bwd_gqa(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dqkv.data_ptr(), 0, B, T,
                                   H, Hkv, hd, hd ** -0.5, ws.data_ptr(), ws.numel() * ws.element_size(), st), "bwd")
    bwd = A.last_launch()
    assert (fwd.path, fwd.kernels, fwd.launches[0].grid) == ("fwd_rows32_gqa", (f"attn_fwd32_gqa_kernel<{hd}>",), B * H * nqb)
    assert (bwd.path, bwd.kernels) == BWD[hd], bwd
    assert [l.grid for l in bwd.launches[1:]] == [[B * (Hkv + H) * nqb], [B * Hkv * nqb, B * H * nqb]][hd == 128]
    # the 32-row multi-head kernels on the [3, H, hd] layout with every K/V head repeated for its group
    q, k, v = qkv.split(w, -1)
    kr, vr = (t.view(B, T, Hkv, hd).repeat_interleave(H // Hkv, 2).view(B, T, H * hd) for t in (k, v))
    rep = torch.cat([q, kr, vr], -1).contiguous()
    o0, lse0 = A.attn_fwd(rep, H, flags=A.FwdFlags.ROUND4 if hd == 64 else 0)
    assert A.last_launch().kernels == (f"attn_fwd32_kernel<{hd}>",)
    d0 = A.attn_bwd(rep, o0, lse0, do, H, flags=A.BwdFlags.FORCE_MERGED if hd == 64 else 0)
    assert A.last_launch().path == ("bwd_rows32_merged" if hd == 64 else "bwd_rows32_128")
    assert torch.equal(o, o0) and torch.equal(lse, lse0) and torch.equal(dqkv[..., :H * hd], d0[..., :H * hd])
    assert Hkv < H or torch.equal(dqkv, d0)
    for name, t, r in zip(("dk", "dv"), dqkv.split(w, -1)[1:], ref64(qkv, do, H, Hkv, hd)):
        _close_blocks(t.view(B, T, Hkv, hd), r, 3e-2, BLOCK, 1, name)


@pytest.mark.parametrize("H,Hkv,hd,T", [(4, 2, 64, 328), (6, 2, 128, 200)])
def test_deterministic_and_graph_replay(cuda, H, Hkv, hd, T):
    qkv, do = _r(B, T, (H + 2 * Hkv) * hd, seed=34), _r(B, T, H * hd, seed=35)

    def run():
        o, lse = A.attn_fwd(qkv, H, n_kv_heads=Hkv)
        return o, lse, A.attn_bwd(qkv, o, lse, do, H, n_kv_heads=Hkv)

    first, again = run(), run()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin(capture_error_mode="thread_local")
        captured = run()
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    for t in captured:
        t.fill_(-7.25)
    g.replay()
    torch.cuda.synchronize()
    for name, x, y, z in zip(("o", "lse", "dqkv"), first, again, captured):
        assert torch.equal(x, y) and torch.equal(x, z), f"{name}: a second run or the graph replay differs"


def test_refusals(cuda):
    T = 64
    A.attn_fwd(_r(1, T, 3 * 2 * 64, seed=3), 2)  # something to leave in the record
    before = A.last_launch()
    for H, Hkv, hd in ((4, 2, 32), (4, 3, 64)):  # head_dim 32; H % Hkv != 0
        qkv, do = _r(1, T, (H + 2 * Hkv) * hd, seed=1), _r(1, T, H * hd, seed=2)
        for call in (lambda: A.attn_fwd(qkv, H, n_kv_heads=Hkv), lambda: A.plan_fwd(1, T, H, hd, n_kv_heads=Hkv),
                     lambda: A.attn_bwd(qkv, do, torch.zeros(1, H, T, device=cuda), do, H, n_kv_heads=Hkv),
                     lambda: A.plan_bwd(1, T, H, hd, n_kv_heads=Hkv)):
            with pytest.raises(RuntimeError, match="4006"):
                call()
    doc = (torch.zeros(1, T, dtype=torch.int32, device=cuda), torch.full((1, T), T, dtype=torch.int32, device=cuda))
    f32, z = _r(1, T, 8 * 64, seed=1, dtype=torch.float32), torch.zeros(1, T, 256, device=cuda)
    for call in (lambda: A.attn_fwd(_r(1, T, 8 * 64, seed=1), 4, n_kv_heads=2, doc=doc),
                 lambda: A.attn_fwd(f32, 4, n_kv_heads=2),
                 lambda: A.attn_bwd(f32, z, torch.zeros(1, 4, T, device=cuda), z, 4, n_kv_heads=2)):
        with pytest.raises(NotImplementedError):
            call()
    assert A.last_launch() == before
