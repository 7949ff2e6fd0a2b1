"""The RMSNorm kernels (csrc/rmsnorm.hip) against float64: forward, both residual-add forms and the backward, on rows with
a large mean, where an RMS statistic differs most from a LayerNorm one.

Widths: 64 one partly filled chunk, 768 GPT-2 small, 1028 ragged in the last chunk, 1536 / 1540 the backward's narrow /
wide cut-off, 2048 / 2052 a power of two (GPT 1.3B) and the first ragged width on the 3-chunk wide backward, 4096 / 4100
the forward's cut-off, 5120 no power of two on 8 waves with a ragged last wave, 8192 the cap.  Metrics and tolerances are
those of tests/test_layernorm_wide_gpu.py (helpers copied, not imported); every row is checked."""

import pytest
import torch

from distributed_training_compare_jax_amd.ops import rmsnorm as RN
from distributed_training_compare_jax_amd.ops.reduce import GradReducer

pytestmark = pytest.mark.gpu

WIDTHS = [64, 768, 1028, 1536, 1540, 2048, 2052, 4096, 4100, 5120, 8192]
EPS = 1e-6
ROWS = ((0.0, 1.0), (100.0, 0.1), (-30.0, 0.05), (1000.0, 1.0), (0.0, 1e-3))  # (c, s): x[m] = c + s * randn(D)


def _r(*shape, scale=1.0, dev="cuda", seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale + 0.1 * torch.rand(*shape, generator=g))
    return t.to(dev).to(dtype)


def _close(a, b, rtol, name=""):
    a, b = a.double().cpu(), b.double().cpu()
    err, ref = (a - b).abs().max().item(), b.abs().max().item() + 1e-6
    print(f"RMS | {name} | max abs err / max {err / ref:.3e} (rtol {rtol:.0e})")
    assert err <= rtol * ref, f"{name}: max abs err {err:.3e} vs ref max {ref:.3e} (rel {err / ref:.2e})"


def _close_rows(out, ref64, rtol, name):
    """``_close`` for every row on its own: max|out-ref| <= rtol * max|ref| within the row."""
    err = (out.detach().cpu().double() - ref64).abs().amax(-1)
    ref = ref64.abs().amax(-1)
    ratio = err / ref.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"RMS | {name} | worst row max abs err / row max {ratio[i].item():.3e} (rtol {rtol:.0e})")
    assert bool((err <= rtol * ref).all()), (f"{name}: worst row {i}: {ratio[i].item():.3e} > rtol {rtol:.1e} "
                                             f"({int((err > rtol * ref).sum())} of {err.numel()} rows over)")


def _offset_rows(M, D, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([ROWS[m % len(ROWS)][0] for m in range(M)])
    s = torch.tensor([ROWS[m % len(ROWS)][1] for m in range(M)])
    return c[:, None] + s[:, None] * torch.randn(M, D, generator=g)


def _check_fwd(x, g, y, rstd, name):
    x = x.detach().cpu().double()
    rr = torch.rsqrt(x.pow(2).mean(-1) + EPS)
    rel = ((rstd.cpu().double() - rr).abs() / rr).max().item()
    print(f"RMS | {name} | rstd rel err {rel:.3e}")
    assert rel <= 1e-4, f"{name}: rstd off by {rel:.3e} relative"
    _close_rows(y, x * rr[:, None] * g.cpu().double(), 1e-2 if y.dtype == torch.bfloat16 else 1e-4, name + " y")


def _bwd_ref64(dy, x, g, rstd, dres):
    """RMSNorm backward in float64 from the fp32 rstd the kernel is given -> (dx, dgamma)."""
    dy, rstd = dy.detach().cpu().double(), rstd.cpu().double()[:, None]
    xhat, gdy = x.cpu().double() * rstd, dy * g.cpu().double()
    dx = (gdy - xhat * (gdy * xhat).mean(-1, keepdim=True)) * rstd
    return (dx if dres is None else dx + dres.cpu().double()), (dy * xhat).sum(0)


@pytest.mark.parametrize("D", WIDTHS)
def test_rmsnorm_offset_rows(cuda, D):
    M = 256
    x, g = _offset_rows(M, D, seed=70), _r(D, dtype=torch.float32, seed=13)
    xd = x.to(cuda)
    y, rs = RN.rmsnorm_fwd(xd, g, EPS, torch.bfloat16)
    _check_fwd(x, g, y, rs, f"rmsnorm_fwd D={D}")
    d = _r(M, D, dtype=torch.float32, seed=71, dev="cpu") * 0.01
    for dd in (d, d.to(torch.bfloat16)):
        want = dd.float() + x
        xs, (y2, rs2) = RN.add_rmsnorm_fwd(dd.to(cuda), xd, g, EPS, torch.bfloat16)
        assert torch.equal(xs.cpu(), want)
        _check_fwd(want, g, y2, rs2, f"add_rmsnorm_fwd {str(dd.dtype)[6:]} D={D}")
    dy, dres = _r(M, D, seed=15), _r(M, D, dtype=torch.float32, seed=16)
    dg, dxc = torch.zeros(D, device=cuda), torch.empty(M, D, dtype=torch.bfloat16, device=cuda)
    dx = RN.rmsnorm_bwd(dy, xd, g, rs, dres, dg, 0.0, out_c=dxc)
    dxr, dgr = _bwd_ref64(dy, x, g, rs, dres)
    _close_rows(dx, dxr, 1e-4, f"rmsnorm_bwd dx D={D}")
    _close_rows(dxc, dxr, 1e-2, f"rmsnorm_bwd dx bf16 D={D}")
    _close(dg, dgr, 1e-4, f"rmsnorm_bwd dgamma D={D}")


@pytest.mark.parametrize("D", [64, 8192])
def test_rmsnorm_ragged_rows_fp32(cuda, D):
    """M = 37, fp32 y and dy, two slabs accumulated onto non-zero gradients, dx written over dres; the rows past M of
    guard-padded outputs stay untouched."""
    M, PAD, GUARD = 37, 8, 768.0  # exact in bf16
    x, g = _offset_rows(M, D, seed=72), _r(D, dtype=torch.float32, seed=13)
    xd = x.to(cuda)
    y, rs = RN.rmsnorm_fwd(xd, g, EPS, torch.float32)
    assert y.dtype == torch.float32
    _check_fwd(x, g, y, rs, f"rmsnorm_fwd fp32 y M={M} D={D}")
    dy, dres = _r(M, D, dtype=torch.float32, seed=15), _r(M, D, dtype=torch.float32, seed=16)
    buf = torch.full((M + PAD, D), GUARD, dtype=torch.float32, device=cuda)
    buf[:M] = dres
    bufc = torch.full((M + PAD, D), GUARD, dtype=torch.bfloat16, device=cuda)
    acc0 = [_r(D, dtype=torch.float32, seed=28 + i) for i in range(2)]
    dg, dbias = (a.clone() for a in acc0)
    dx = RN.rmsnorm_bwd(dy, xd, g, rs, buf[:M], dg, 1.0, out=buf[:M], out_c=bufc[:M], dbias=dbias)
    assert dx.data_ptr() == buf.data_ptr()
    dxr, dgr = _bwd_ref64(dy, x, g, rs, dres)
    _close_rows(dx, dxr, 1e-4, f"rmsnorm_bwd dx M={M} D={D}")
    _close_rows(bufc[:M], dxr, 1e-2, f"rmsnorm_bwd dx bf16 M={M} D={D}")
    _close(dg, acc0[0].cpu().double() + dgr, 1e-4, "dgamma (accumulated)")
    _close(dbias, acc0[1].cpu().double() + dxr.sum(0), 1e-4, "dbias (accumulated)")
    assert bool((buf[M:] == GUARD).all()) and bool((bufc[M:].float() == GUARD).all()), "rows past M were written"


def test_rmsnorm_bwd_reducer_bitwise_and_deterministic(cuda):
    """The deferred partials summed by the batched reducer equal the direct slab reduction bit for bit, for beta 0 and
    1, and two runs of each are bitwise equal."""
    M, D = 256, 2048
    red = GradReducer(cuda, arena_mb=64)
    x, g = _r(M, D, dtype=torch.float32, seed=25), _r(D, dtype=torch.float32, seed=26)
    rs, dy = torch.rsqrt(x.pow(2).mean(-1) + EPS), _r(M, D, dtype=torch.float32, seed=27)
    for beta in (0.0, 1.0):
        outs = []
        for r in (None, None, red, red):
            dg, dbias = (_r(D, dtype=torch.float32, seed=28 + i) for i in range(2))
            outs.append((RN.rmsnorm_bwd(dy, x, g, rs, None, dg, beta, dbias=dbias, red=r), dg, dbias))
        assert red.pending, "tasks should be queued until flush"
        red.flush()
        for o in outs[1:]:
            for a, b, name in zip(outs[0], o, ("dx", "dgamma", "dbias")):
                assert torch.equal(a, b), f"rmsnorm_bwd: {name}, beta {beta}"
        assert float(outs[0][1].abs().max()) > 0


@pytest.mark.parametrize("D", [8196, 2050])
def test_rmsnorm_refuses_bad_widths(cuda, D):
    """D > 8192 or D % 4 != 0 raises from every entry point before anything is launched; a valid call right after
    works."""
    M = 8
    x, g = _r(M, D, dtype=torch.float32, seed=1), _r(D, dtype=torch.float32, seed=2)
    with pytest.raises(RuntimeError, match="dtc_rmsnorm_fwd"):
        RN.rmsnorm_fwd(x, g, EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_add_rmsnorm_fwd "):
        RN.add_rmsnorm_fwd(x.clone(), x, g, EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_add_rmsnorm_fwd_bf16"):
        RN.add_rmsnorm_fwd(x.to(torch.bfloat16), x, g, EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_rmsnorm_bwd"):
        RN.rmsnorm_bwd(x.to(torch.bfloat16), x, g, x.mean(-1), None, torch.zeros(D, device=cuda))
    torch.cuda.synchronize()
    x = _offset_rows(M, 2052, seed=5)
    g = _r(2052, dtype=torch.float32, seed=2)
    y, rs = RN.rmsnorm_fwd(x.to(cuda), g, EPS, torch.bfloat16)
    torch.cuda.synchronize()
    _check_fwd(x, g, y, rs, "rmsnorm_fwd after a refusal")
