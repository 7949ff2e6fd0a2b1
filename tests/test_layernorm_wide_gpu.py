"""The wide LayerNorm kernels (csrc/norm_reduce.hip ln_fwd_wide_kernel / ln_bwd_wide_kernel): forward
2048 < D <= 8192, backward 1024 < D <= 8192, a row spread over the waves of a block.

Widths: 1028 is the first past the old backward limit (ragged in the last column chunk, one wave of the block
without a column), 2048 the widest forward of the old kernel next to the new backward, 2052 the first past the
old forward limit, 5120 no power of two and the first width on 8 waves per block with a ragged last wave, 8192
the cap.  The float64 references, metrics and tolerances are those of
tests/test_kernels_scale_gpu.py::test_layernorm_offset_rows (copied, not imported); they do not depend on D: the
deepest sum is 8192 fp32 terms.

``tests/golden/ln_narrow_parent.npz`` pins the kernels the old widths keep: the outputs of ``_pinned_outputs``
recorded on an MI355X with the library built from the commit before the wide kernels (``DTC_KERNEL_LIB`` pointing
at that build, ``numpy.savez_compressed`` of the dictionary).
"""

import os

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.ops import layernorm as LN
from distributed_training_compare_jax_amd.ops.reduce import GradReducer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_narrow_parent.npz")
WIDTHS = [1028, 2048, 2052, 5120, 8192]
LN_EPS = 1e-6
LN_ROWS = ((0.0, 1.0), (100.0, 0.1), (-30.0, 0.05), (1000.0, 1.0), (0.0, 1e-3))  # (c, s): x[m] = c + s * randn(D)


# ------------------------------------------------------- helpers of tests/test_kernels_(scale_)gpu.py (copies)

def _r(*shape, scale=1.0, dev="cuda", seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale + 0.1 * torch.rand(*shape, generator=g))
    return t.to(dev).to(dtype)


def _close(a, b, rtol, name=""):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= rtol * ref, f"{name}: max abs err {err:.3e} vs ref max {ref:.3e} (rel {err / ref:.2e})"


def _close_rows(out, ref64, rtol, name, rows=None):
    """``_close`` for every row on its own: max|out-ref| <= rtol * max|ref| within the row."""
    err = (out.detach().cpu().double() - ref64).abs().amax(-1)
    ref = ref64.abs().amax(-1)
    if rows is not None:
        err, ref = err[rows], ref[rows]
    ratio = err / ref.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"WIDE-LN | {name} | worst row max abs err / row max {ratio[i].item():.3e} (rtol {rtol:.0e})")
    assert bool((err <= rtol * ref).all()), (
        f"{name}: worst row {i if rows is None else int(torch.nonzero(rows)[i])}: max abs err / row max = "
        f"{ratio[i].item():.3e} > rtol {rtol:.1e} ({int((err > rtol * ref).sum())} of {err.numel()} rows over)")


def _offset_rows(M, D, seed):
    """fp32 rows cycling over LN_ROWS: a residual stream that drifted away from 0.  Returns (x, c)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([LN_ROWS[m % len(LN_ROWS)][0] for m in range(M)])
    s = torch.tensor([LN_ROWS[m % len(LN_ROWS)][1] for m in range(M)])
    return c[:, None] + s[:, None] * torch.randn(M, D, generator=g), c


def _ln_ref64(x, g, b):
    x = x.detach().cpu().double()
    mean = x.mean(-1)
    rstd = torch.rsqrt((x - mean[:, None]).pow(2).mean(-1) + LN_EPS)
    xhat = (x - mean[:, None]) * rstd[:, None]
    return mean, rstd, xhat, xhat * g.cpu().double() + b.cpu().double()


def _y_rows(x):
    """Rows whose y is checked at 1e-2: those where an fp32 two-pass LayerNorm on the CPU keeps xhat within 1e-3
    of float64 -- a condition on the input alone."""
    x = x.detach().cpu()
    mean = x.mean(-1, keepdim=True)
    xhat = (x - mean) * torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + LN_EPS)
    return (xhat.double() - _ln_ref64(x, torch.ones(1), torch.zeros(1))[2]).abs().amax(-1) < 1e-3


def _check_rstd(rstd, ref64, name):
    rel = ((rstd.detach().cpu().double() - ref64).abs() / ref64).max().item()
    m = int(((rstd.detach().cpu().double() - ref64).abs() / ref64).argmax())
    assert rel <= 1e-4, f"{name}: rstd of row {m} (c, s = {LN_ROWS[m % len(LN_ROWS)]}) off by {rel:.3e} relative > 1e-4"
    return rel


def _check_ln_fwd(x, c, g, b, y, mean, rstd, name):
    """Per row: rstd to 1e-4 relative, mean to 1e-6 |c| + 1e-6, y to 1e-2 of the row's max on the _y_rows rows,
    which at these widths must be all rows."""
    mr, rr, _, yr = _ln_ref64(x, g, b)
    rel = _check_rstd(rstd, rr, name)
    merr = (mean.cpu().double() - mr).abs()
    mtol = 1e-6 * c.abs().double() + 1e-6
    m = int((merr - mtol).argmax())
    print(f"WIDE-LN | {name} | rstd rel err {rel:.3e} | mean err / tol {(merr / mtol).max().item():.3f}")
    assert bool((merr <= mtol).all()), f"{name}: mean of row {m} off by {merr[m]:.3e} > {mtol[m]:.3e}"
    rows = _y_rows(x)
    assert bool(rows[1::len(LN_ROWS)].all()), "the (100, 0.1) rows must be among the checked ones"
    assert bool(rows.all()), f"{name}: _y_rows leaves out {int((~rows).sum())} rows; no row may go unchecked here"
    _close_rows(y, yr, 1e-2, name + " y", rows)


def _ln_bwd_ref64(dy, x, g, mean, rstd, dres):
    """LayerNorm backward in float64 from the fp32 mean / rstd the kernel is given."""
    dy, g = dy.detach().cpu().double(), g.cpu().double()
    rstd = rstd.cpu().double()[:, None]
    xhat = (x.cpu().double() - mean.cpu().double()[:, None]) * rstd
    gdy = dy * g
    dx = (gdy - gdy.mean(-1, keepdim=True) - xhat * (gdy * xhat).mean(-1, keepdim=True)) * rstd
    if dres is not None:
        dx = dx + dres.cpu().double()
    return dx, (dy * xhat).sum(0), dy.sum(0)


# ------------------------------------------------------------------------------------------------ the tests

@pytest.mark.parametrize("D", WIDTHS)
def test_wide_layernorm_offset_rows(cuda, D):
    """layernorm_fwd, add_layernorm_fwd (fp32 and bf16 d) and layernorm_bwd with dres and out_c on rows with a
    large mean, against float64."""
    M = 256
    x, c = _offset_rows(M, D, seed=70)
    g, b = _r(D, dtype=torch.float32, seed=13), _r(D, dtype=torch.float32, seed=14)
    xd = x.to(cuda)
    y, mu, rs = LN.layernorm_fwd(xd, g, b, LN_EPS, torch.bfloat16)
    _check_ln_fwd(x, c, g, b, y, mu, rs, f"layernorm_fwd D={D}")
    d = _r(M, D, dtype=torch.float32, seed=71, dev="cpu") * 0.01
    for dd in (d, d.to(torch.bfloat16)):
        want = dd.float() + x
        xs, (y2, mu2, rs2) = LN.add_layernorm_fwd(dd.to(cuda), xd, g, b, LN_EPS, torch.bfloat16)
        assert torch.equal(xs.cpu(), want)
        _check_ln_fwd(want, c, g, b, y2, mu2, rs2, f"add_layernorm_fwd {str(dd.dtype)[6:]} D={D}")
    dy, dres = _r(M, D, seed=15), _r(M, D, dtype=torch.float32, seed=16)
    dg, db = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
    dxc = torch.empty(M, D, dtype=torch.bfloat16, device=cuda)
    dx = LN.layernorm_bwd(dy, xd, g, mu, rs, dres, dg, db, 0.0, out_c=dxc)
    dxr, dgr, dbr = _ln_bwd_ref64(dy, x, g, mu, rs, dres)
    _close_rows(dx, dxr, 1e-4, f"layernorm_bwd dx D={D}")
    _close_rows(dxc, dxr, 1e-2, f"layernorm_bwd dx bf16 D={D}")
    _close(dg.cpu(), dgr, 1e-4, "layernorm_bwd dgamma")
    _close(db.cpu(), dbr, 1e-4, "layernorm_bwd dbeta")


@pytest.mark.parametrize("D", [1028, 8192])
def test_wide_layernorm_ragged_rows_fp32(cuda, D):
    """M = 37 (no multiple of any rows-per-group or rows-per-block), the exact-fp32 mode's types (fp32 y and dy),
    three slabs accumulated onto non-zero gradients, dx written over dres; the rows past M of guard-padded
    outputs stay untouched."""
    M, PAD, GUARD = 37, 8, 768.0  # exact in bf16
    x, c = _offset_rows(M, D, seed=72)
    g, b = _r(D, dtype=torch.float32, seed=13), _r(D, dtype=torch.float32, seed=14)
    xd = x.to(cuda)
    y, mu, rs = LN.layernorm_fwd(xd, g, b, LN_EPS, torch.float32)
    assert y.dtype == torch.float32
    _check_ln_fwd(x, c, g, b, y, mu, rs, f"layernorm_fwd fp32 y M={M} D={D}")
    dy, dres = _r(M, D, dtype=torch.float32, seed=15), _r(M, D, dtype=torch.float32, seed=16)
    buf = torch.full((M + PAD, D), GUARD, dtype=torch.float32, device=cuda)
    buf[:M] = dres
    bufc = torch.full((M + PAD, D), GUARD, dtype=torch.bfloat16, device=cuda)
    acc0 = [_r(D, dtype=torch.float32, seed=28 + i) for i in range(3)]
    dg, db, dbias = (a.clone() for a in acc0)
    dx = LN.layernorm_bwd(dy, xd, g, mu, rs, buf[:M], dg, db, 1.0, out=buf[:M], out_c=bufc[:M], dbias=dbias)
    assert dx.data_ptr() == buf.data_ptr()
    dxr, dgr, dbr = _ln_bwd_ref64(dy, x, g, mu, rs, dres)
    _close_rows(dx, dxr, 1e-4, f"layernorm_bwd dx M={M} D={D}")
    _close_rows(bufc[:M], dxr, 1e-2, f"layernorm_bwd dx bf16 M={M} D={D}")
    _close(dg.cpu(), acc0[0].cpu().double() + dgr, 1e-4, "dgamma (accumulated)")
    _close(db.cpu(), acc0[1].cpu().double() + dbr, 1e-4, "dbeta (accumulated)")
    _close(dbias.cpu(), acc0[2].cpu().double() + dxr.sum(0), 1e-4, "dbias (accumulated)")
    assert bool((buf[M:] == GUARD).all()) and bool((bufc[M:].float() == GUARD).all()), "rows past M were written"


def test_wide_layernorm_bwd_via_reducer_is_bitwise(cuda):
    """The deferred partials summed by the batched reducer equal the direct slab reduction bit for bit."""
    M, D = 256, 2048
    red = GradReducer(cuda, arena_mb=64)
    xx, g = _r(M, D, dtype=torch.float32, seed=25), _r(D, dtype=torch.float32, seed=26)
    mu, rs = xx.mean(-1), torch.rsqrt(xx.var(-1, unbiased=False) + 1e-6)
    dyl = _r(M, D, dtype=torch.float32, seed=27)
    for beta in (0.0, 1.0):
        outs = []
        for r in (None, red):
            dg, dbb, dbias = (_r(D, dtype=torch.float32, seed=28 + i) for i in range(3))
            dx = LN.layernorm_bwd(dyl, xx, g, mu, rs, None, dg, dbb, beta, dbias=dbias, red=r)
            outs.append((dx, dg, dbb, dbias))
        assert red.pending, "tasks should be queued until flush"
        red.flush()
        for a, b, name in zip(*outs, ("dx", "dgamma", "dbeta", "dbias")):
            assert torch.equal(a, b), f"layernorm_bwd via reducer: {name}, beta {beta}"
        assert float(outs[0][1].abs().max()) > 0


def test_wide_layernorm_bwd_is_deterministic(cuda):
    M, D = 256, 5120
    x, g = _r(M, D, dtype=torch.float32, seed=25), _r(D, dtype=torch.float32, seed=26)
    mu, rs = x.mean(-1), torch.rsqrt(x.var(-1, unbiased=False) + 1e-6)
    dy, dres = _r(M, D, seed=27), _r(M, D, dtype=torch.float32, seed=16)
    runs = []
    for _ in range(2):
        dg, db = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
        dxc = torch.empty(M, D, dtype=torch.bfloat16, device=cuda)
        dx = LN.layernorm_bwd(dy, x, g, mu, rs, dres, dg, db, 0.0, out_c=dxc)
        runs.append((dx, dxc, dg, db))
    for a, b, name in zip(*runs, ("dx", "dx bf16", "dgamma", "dbeta")):
        assert torch.equal(a, b), name


def _pinned_outputs():
    """The narrow kernels at their widest: forward D = 2048 (plain and bf16-d residual form), backward D = 1024
    (bf16 dy, dres, bf16 copy, three slabs).  M = 64, fixed seeds."""
    M = 64
    out = {}
    D = 2048
    x, g, b = _r(M, D, dtype=torch.float32, seed=41), _r(D, dtype=torch.float32, seed=42), _r(D, dtype=torch.float32, seed=43)
    y, mu, rs = LN.layernorm_fwd(x, g, b, LN_EPS, torch.bfloat16)
    out.update(fwd_y=y, fwd_mean=mu, fwd_rstd=rs)
    d = _r(M, D, seed=44)
    _, (y, mu, rs) = LN.add_layernorm_fwd(d, x, g, b, LN_EPS, torch.bfloat16)
    out.update(add_y=y, add_mean=mu, add_rstd=rs)
    D = 1024
    x, g = _r(M, D, dtype=torch.float32, seed=45), _r(D, dtype=torch.float32, seed=46)
    mu, rs = x.mean(-1), torch.rsqrt(x.var(-1, unbiased=False) + 1e-6)
    dy, dres = _r(M, D, seed=47), _r(M, D, dtype=torch.float32, seed=48)
    dg, db, dbias = (torch.zeros(D, device=x.device) for _ in range(3))
    dxc = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    dx = LN.layernorm_bwd(dy, x, g, mu, rs, dres, dg, db, 0.0, out_c=dxc, dbias=dbias)
    out.update(bwd_dx=dx, bwd_dxc=dxc, bwd_dg=dg, bwd_db=db, bwd_dbias=dbias, bwd_mean=mu, bwd_rstd=rs)
    torch.cuda.synchronize()
    # bf16 has no numpy type: stored as its 16 bits
    return {k: (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).cpu().numpy() for k, v in out.items()}


def test_narrow_widths_unchanged(cuda):
    """D = 2048 forward and D = 1024 backward still run the old kernels: bitwise the recorded outputs."""
    want = np.load(GOLDEN)
    got = _pinned_outputs()
    assert sorted(want.files) == sorted(got)
    # the inputs of the backward come from torch reductions: if those differ from the recording, the comparison
    # below says nothing about the kernel
    for k in ("bwd_mean", "bwd_rstd"):
        assert np.array_equal(got[k], want[k]), f"{k}: the test's own inputs differ from the recording"
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{k} differs from the parent's kernel"


@pytest.mark.parametrize("D", [8196, 2050])
def test_wide_layernorm_refuses_bad_widths(cuda, D):
    """D > 8192 or D % 4 != 0 raises from all four entry points before anything is launched; a valid call right
    after works and the device reports no error."""
    M = 8
    x = _r(M, D, dtype=torch.float32, seed=1)
    g, b = _r(D, dtype=torch.float32, seed=2), _r(D, dtype=torch.float32, seed=3)
    mu, rs = x.mean(-1), torch.rsqrt(x.var(-1, unbiased=False) + 1e-6)
    with pytest.raises(RuntimeError, match="dtc_layernorm_fwd"):
        LN.layernorm_fwd(x, g, b, LN_EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_add_layernorm_fwd "):
        LN.add_layernorm_fwd(x.clone(), x, g, b, LN_EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_add_layernorm_fwd_bf16"):
        LN.add_layernorm_fwd(x.to(torch.bfloat16), x, g, b, LN_EPS, torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtc_layernorm_bwd"):
        LN.layernorm_bwd(x.to(torch.bfloat16), x, g, mu, rs, None, torch.zeros(D, device=cuda),
                         torch.zeros(D, device=cuda))
    torch.cuda.synchronize()
    D = 2052
    x, c = _offset_rows(M, D, seed=5)
    g, b = _r(D, dtype=torch.float32, seed=2), _r(D, dtype=torch.float32, seed=3)
    y, mu, rs = LN.layernorm_fwd(x.to(cuda), g, b, LN_EPS, torch.bfloat16)
    torch.cuda.synchronize()
    _check_ln_fwd(x, c, g, b, y, mu, rs, "layernorm_fwd after a refusal")
