"""The fused QK-norm + RoPE kernels (csrc/qknorm.hip) against float64, per head: forward (y, rstd, the raw copy),
backward (dx, both gain gradients), with and without the table, bf16 and fp32.

Cases (H, Hkv, hd): a partly filled pass, more than one pass in both dtypes, passes that straddle the Q / K boundary.
Heads are c + s * randn with the (c, s) of tests/test_rmsnorm_gpu.py; dy is 16 times larger on one query head per group
and on key head 0, so a lost or swapped head misses by orders of magnitude.  Metric and bounds are that file's, per head:
max|out - ref| <= rtol * max|ref| within the head (docs/NUMERICS.md); the backward reference starts from the kernel's rstd."""

import pytest
import torch

from distributed_training_compare_jax_amd.ops.qknorm import qknorm_rope_bwd_, qknorm_rope_fwd_
from distributed_training_compare_jax_amd.ops.reduce import GradReducer
from distributed_training_compare_jax_amd.ops.rope import rope_table

pytestmark = pytest.mark.gpu

EPS = 1e-6
ROWS = ((0.0, 1.0), (100.0, 0.1), (-30.0, 0.05), (1000.0, 1.0), (0.0, 1e-3))  # (c, s): head = c + s * randn(hd)
CASES = [(2, 2, 32), (40, 8, 32), (4, 2, 64), (3, 1, 64), (20, 4, 64), (6, 2, 128), (8, 2, 128), (5, 5, 128)]


def _inputs(B, T, H, Hkv, hd, dtype, seed=0, ones=False):
    g = torch.Generator().manual_seed(seed)
    n = H + 2 * Hkv
    idx = torch.arange(B * T * n).view(B, T, n) % len(ROWS)
    c, s = torch.tensor([r[0] for r in ROWS])[idx], torch.tensor([r[1] for r in ROWS])[idx]
    x = (c[..., None] + s[..., None] * torch.randn(B, T, n, hd, generator=g)).view(B, T, n * hd).to(dtype)
    gq, gk = ((torch.ones(hd) if ones else torch.randn(hd, generator=g)) for _ in range(2))
    scale, G = torch.ones(n), H // Hkv
    scale[[grp * G + grp % G for grp in range(Hkv)] + [H]] = 16.0
    dy = (torch.randn(B, T, n, hd, generator=g) * scale[:, None]).view(B, T, n * hd).to(dtype)
    return x, gq, gk, dy


def _rot64(z, tab, T, sign):
    if tab is None:
        return z
    hd = z.shape[-1]
    c, s = tab[:T, :, 0].double().cpu()[None, :, None], sign * tab[:T, :, 1].double().cpu()[None, :, None]
    lo, hi = z[..., :hd // 2], z[..., hd // 2:]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)


def _ref64(x, gq, gk, dy, rstd, tab, H, Hkv, hd):  # float64 (rstd, y, dx, dgq, dgk); the backward from the kernel's rstd
    B, T, nrot = x.shape[0], x.shape[1], H + Hkv
    x64 = x.double()[..., :nrot * hd].view(B, T, nrot, hd)
    g = torch.cat([gq.double().expand(H, hd), gk.double().expand(Hkv, hd)])
    rr = torch.rsqrt(x64.pow(2).mean(-1) + EPS)
    y = _rot64(x64 * rr[..., None] * g, tab, T, 1.0)
    rs = rstd.double().cpu()[..., None]
    dz = _rot64(dy.double()[..., :nrot * hd].view(B, T, nrot, hd), tab, T, -1.0)
    xh, dxh = x64 * rs, dz * g
    dx = rs * (dxh - xh * (dxh * xh).mean(-1, keepdim=True))
    p = dz * xh
    return rr, y, dx, p[:, :, :H].sum((0, 1, 2)), p[:, :, H:].sum((0, 1, 2))


def _close_heads(out, ref, rtol, name):
    out = out.double().cpu().view(ref.shape)
    err, mx = (out - ref).abs().amax(-1), ref.abs().amax(-1)
    worst = (err / mx.clamp_min(1e-300)).max().item()
    print(f"QKN | {name} | worst head max abs err / head max {worst:.3e} (rtol {rtol:.0e})")
    assert bool((err <= rtol * mx).all()), f"{name}: worst head {worst:.3e} > {rtol:.0e}"


def _run_and_check(cuda, B, T, H, Hkv, hd, dtype, table):
    tab = rope_table(130, hd, 10000.0, cuda) if table else None
    x, gq, gk, dy = _inputs(B, T, H, Hkv, hd, dtype)
    n, rtol = (H + Hkv) * hd, 1e-2 if dtype == torch.bfloat16 else 1e-4
    xd, gqd, gkd = x.to(cuda), gq.to(cuda), gk.to(cuda)
    y, raw, rstd = qknorm_rope_fwd_(xd.clone(), tab, gqd, gkd, H, Hkv, EPS)
    rr, yr, dxr, dgq_r, dgk_r = _ref64(x, gq, gk, dy, rstd, tab, H, Hkv, hd)
    assert torch.equal(raw.cpu(), x[..., :n]), "qk_raw is not the input's Q | K columns bit for bit"
    assert torch.equal(y[..., n:].cpu(), x[..., n:]), "the V columns changed"
    _close_heads(rstd[..., None], rr[..., None], 1e-4, "rstd")  # one element per "head": the relative error
    _close_heads(y[..., :n], yr, rtol, "y")
    dgq, dgk = torch.full((hd,), 7.0, device=cuda), torch.full((hd,), 7.0, device=cuda)  # beta 0 overwrites
    dx = qknorm_rope_bwd_(dy.to(cuda), tab, raw, rstd, gqd, gkd, H, Hkv, dgq, dgk)
    assert torch.equal(dx[..., n:].cpu(), dy[..., n:]), "the V columns of dqkv changed"
    _close_heads(dx[..., :n], dxr, rtol, "dx")
    _close_heads(dgq, dgq_r, 1e-4, "dg_q")  # a vector is one "head": 1e-4 of its maximum
    _close_heads(dgk, dgk_r, 1e-4, "dg_k")


@pytest.mark.parametrize("table", [True, False], ids=["rope", "notab"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
# B * T: 2 rows (half a forward block), 144 = 4 backward blocks of 32 and one of 16, 260 = 8 and one of 4
@pytest.mark.parametrize("T", [1, 72, 130])
@pytest.mark.parametrize("H,Hkv,hd", CASES)
def test_qknorm_matches_float64(cuda, H, Hkv, hd, T, dtype, table):
    _run_and_check(cuda, 2, T, H, Hkv, hd, dtype, table)


def test_beta_reducer_repeat_and_graph_replay(cuda):
    """Gains 1, no table: beta = 1 adds the beta = 0 reduction exactly; GradReducer, a second run and replays repeat it."""
    B, T, H, Hkv, hd = 2, 72, 4, 2, 64
    x, gq, gk, dy = (t.to(cuda) for t in _inputs(B, T, H, Hkv, hd, torch.bfloat16, seed=1, ones=True))

    def run(beta, red=None, init=0.0):
        dgq, dgk = torch.full((hd,), init, device=cuda), torch.full((hd,), -init, device=cuda)
        y, raw, rstd = qknorm_rope_fwd_(x.clone(), None, gq, gk, H, Hkv, EPS)
        dx = qknorm_rope_bwd_(dy.clone(), None, raw, rstd, gq, gk, H, Hkv, dgq, dgk, beta, red=red)
        if red is not None:
            red.flush()
        return y, raw, rstd, dx, dgq, dgk

    first = run(0.0)
    assert float(first[4].abs().max()) > 0 and float(first[5].abs().max()) > 0
    acc = run(1.0, init=3.0)
    assert torch.equal(acc[4], 3.0 + first[4]) and torch.equal(acc[5], -3.0 + first[5])
    red = GradReducer(cuda, arena_mb=16)
    for other, beta, want in ((run(0.0), 0.0, first), (run(0.0, red), 0.0, first), (run(1.0, red, 3.0), 1.0, acc)):
        for a, b in zip(want, other):
            assert torch.equal(a, b), f"beta {beta}"
    torch.cuda.synchronize()
    xb, db = x.clone(), dy.clone()
    dgq, dgk = torch.zeros(hd, device=cuda), torch.zeros(hd, device=cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, raw, rstd = qknorm_rope_fwd_(xb, None, gq, gk, H, Hkv, EPS)
        qknorm_rope_bwd_(db, None, raw, rstd, gq, gk, H, Hkv, dgq, dgk)
    for _ in range(3):
        xb.copy_(x)
        db.copy_(dy)
        graph.replay()
        for a, b in zip(first, (xb, raw, rstd, db, dgq, dgk)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["heads", "head_dim", "table", "align"])
def test_refusals_leave_the_tensors_untouched(cuda, case):
    H, Hkv, hd, T = (3, 2, 64, 8) if case == "heads" else (2, 2, 48 if case == "head_dim" else 64, 8)
    tab = rope_table(4 if case == "table" else 16, hd, 10000.0, cuda)
    n = 2 * T * (H + 2 * Hkv) * hd
    buf = torch.randn(n + 8, device=cuda).to(torch.bfloat16)
    off = 1 if case == "align" else 0  # one bf16 element: 2 bytes off a 16-byte boundary
    keep, g = buf.clone(), torch.ones(hd, device=cuda)
    raw = torch.zeros(2, T, (H + Hkv) * hd, dtype=torch.bfloat16, device=cuda)
    rstd, dg = torch.ones(2, T, H + Hkv, device=cuda), torch.full((hd,), 5.0, device=cuda)
    with pytest.raises((RuntimeError, ValueError)):
        qknorm_rope_fwd_(buf[off:off + n].view(2, T, -1), tab, g, g, H, Hkv, EPS)
    with pytest.raises((RuntimeError, ValueError)):
        qknorm_rope_bwd_(buf[off:off + n].view(2, T, -1), tab, raw, rstd, g, g, H, Hkv, dg, dg)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and bool((dg == 5.0).all())
