"""``norm: rmsnorm`` on the CPU: the config field, the torch paths of ``ops/rmsnorm.py`` against float64, one engine step
against ``models/reference.py``, the checkpoint and engine refusals."""

import dataclasses

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import rmsnorm as RN
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.utils import checkpoint as CK

EPS = 1e-6
SHIFT = 0.05  # added to wte (see step_vs_oracle)


def _engine(norm="rmsnorm", **tc):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, n_heads=4, norm=norm)
    cfg = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/unused", device="cpu", **tc)
    return Engine(mc, cfg, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, 1, 0, torch.device("cpu"), "gloo")), mc


def test_config_validation_and_num_params():
    mc = model_config_from_preset("tiny", vocab_size=100)
    assert mc.norm == "layernorm"
    rms = dataclasses.replace(mc, norm="rmsnorm")
    assert mc.num_params() - rms.num_params() == (2 * mc.n_layers + 1) * mc.d_model
    with pytest.raises(ValueError, match="norm"):
        dataclasses.replace(mc, norm="batchnorm")


def test_torch_paths_match_float64():
    g0 = torch.Generator().manual_seed(3)
    M, D = 10, 64
    x, d = 5.0 + torch.randn(M, D, generator=g0), 0.1 * torch.randn(M, D, generator=g0)
    g, dy, dres = (torch.randn(s, generator=g0) for s in ((D,), (M, D), (M, D)))
    x64, g64 = x.double(), g.double()
    rs64 = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS)
    y, rs = RN.rmsnorm_fwd(x, g, EPS)
    assert torch.allclose(y.double(), x64 * rs64 * g64, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rs.double(), rs64[:, 0], rtol=1e-6)
    xs, (y2, rs2) = RN.add_rmsnorm_fwd(d.to(torch.bfloat16), x, g, EPS)
    assert torch.equal(xs, d.to(torch.bfloat16).float() + x) and torch.equal(y2, RN.rmsnorm_fwd(xs, g, EPS)[0])
    xh, gdy = x64 * rs64, dy.double() * g64
    dx64 = (gdy - xh * (gdy * xh).mean(-1, keepdim=True)) * rs64 + dres.double()
    dg, dbias = torch.ones(D), torch.ones(D)
    dx = RN.rmsnorm_bwd(dy, x, g, rs, dres, dg, 1.0, dbias=dbias)
    assert torch.allclose(dx.double(), dx64, rtol=1e-5, atol=1e-5)
    assert torch.allclose(dg.double(), 1 + (dy.double() * xh).sum(0), rtol=1e-5, atol=1e-5)
    assert torch.allclose(dbias.double(), 1 + dx64.sum(0), rtol=1e-5, atol=1e-5)


def step_vs_oracle(eng, mc, b, shift):
    """One forward + backward of ``eng`` on batch ``b`` with ``wte`` shifted by ``shift`` (at initialisation the residual
    rows have almost no mean and the two norms nearly coincide) against autograd through the oracle -> (loss, oracle loss,
    worst relative gradient error, relative distance of the oracle's h.0.qkv.w gradient to the one under layernorm)."""
    eng.flat.p("wte").add_(shift)
    eng.flat.refresh_mirror()
    eng.set_batch(b)
    st, (rows, T), ctx = eng.stage, eng.ids.shape, {}
    h = st.stage_forward(st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx), rows, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (rows * T), ctx).item()
    dx, _ = st.stage_backward(ctx, *st.head_backward(ctx, 1 / (rows * T), 0.0), 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    lo = oracle_loss(mc, params, ids, lab, 0, 0)
    lo.backward()
    ln = {n: p.detach().clone().requires_grad_(True) for n, p in params.items()}
    ln.update({n[:-1] + "b": torch.zeros(mc.d_model) for n in params if n.endswith(("ln1.g", "ln2.g", "lnf.g"))})
    oracle_loss(dataclasses.replace(mc, norm="layernorm"), ln, ids, lab, 0, 0).backward()
    gq = params["h.0.qkv.w"].grad
    worst = max(((eng.flat.g(n).cpu() - params[n].grad).norm() / (params[n].grad.norm() + 1e-12)).item()
                for n in eng.flat.slots)
    return loss, lo.item(), worst, ((gq - ln["h.0.qkv.w"].grad).norm() / gq.norm()).item()


def test_cpu_engine_step_matches_the_oracle():
    eng, mc = _engine()
    assert not [n for n in eng.flat.slots if n.endswith(("ln1.b", "ln2.b", "lnf.b"))] and "h.0.ln1.g" in eng.flat.slots
    loss, lo, worst, gap = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)), SHIFT)
    assert gap > 0.5, f"the oracle's h.0.qkv.w gradient barely depends on the norm ({gap:.3f})"
    assert abs(loss - lo) < 1e-5 and worst < 1e-4, (loss, lo, worst)  # bounds of tests/test_model_cpu.py


def test_checkpoint_resume_under_the_other_norm_raises(tmp_path):
    eng, _ = _engine()
    CK.save(eng, str(tmp_path), 1)
    other, _ = _engine("layernorm")
    with pytest.raises(ValueError, match="norm='rmsnorm'"):
        CK.load_into(other, str(tmp_path), 1)


def test_engine_refuses_rmsnorm_with_mxfp8():
    with pytest.raises(ValueError, match="norm=rmsnorm cannot be combined with fwd_gemm_dtype=mxfp8"):
        _engine(fwd_gemm_dtype="mxfp8")
