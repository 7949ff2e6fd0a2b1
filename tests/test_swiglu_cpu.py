"""``mlp: swiglu`` on the CPU: the config field and what derives from it, the ``glu_rows`` tensor-parallel split, the torch
paths of ``ops/swiglu.py`` against float64 autograd, one engine step against ``models/reference.py``, the refusals."""

import dataclasses

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models import params as P
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import swiglu as SW
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.utils import checkpoint as CK


def _engine(mlp="swiglu", **tc):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, n_heads=4, mlp=mlp)
    cfg = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/unused", device="cpu", **tc)
    return Engine(mc, cfg, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, 1, 0, torch.device("cpu"), "gloo")), mc


def test_config_inventory_num_params_and_flops():
    mc = model_config_from_preset("tiny", vocab_size=100)
    assert mc.mlp == "gelu" and P.all_param_specs(mc) == P.all_param_specs(dataclasses.replace(mc, mlp="gelu"))
    glu = dataclasses.replace(mc, mlp="swiglu")
    D, F, L = mc.d_model, mc.d_ff, mc.n_layers
    count = lambda c: sum(torch.Size(s.shape).numel() for s in P.all_param_specs(c))  # noqa: E731
    by_name = {s.name: s for s in P.all_param_specs(glu)}
    assert by_name["h.0.fc1.w"].shape == (2 * F, D) and by_name["h.0.fc1.b"].shape == (2 * F,)
    assert by_name["h.0.fc2.w"].shape == (D, F) and by_name["h.0.fc1.w"].tp == "glu_rows"
    assert count(glu) - count(mc) == glu.num_params() - mc.num_params() == L * (D * F + F)
    assert glu.flops_per_token() - mc.flops_per_token() == 6.0 * L * D * F  # a third D x F matmul, fwd + bwd
    with pytest.raises(ValueError, match="mlp"):
        dataclasses.replace(mc, mlp="geglu")


@pytest.mark.parametrize("tp", [2, 4])
def test_glu_rows_round_trip_and_sharded_mlp(tp):
    g0 = torch.Generator().manual_seed(tp)
    D, F, M = 16, 24, 5
    mc = model_config_from_preset("tiny", vocab_size=100, d_model=D, d_ff=F, mlp="swiglu")
    spec = {s.name: s for s in P.layer_param_specs(mc, 0)}
    full = {n: torch.randn(spec[n].shape, generator=g0, dtype=torch.float64) for n in ("h.0.fc1.w", "h.0.fc1.b", "h.0.fc2.w")}
    sh = {n: [P.shard(spec[n], t, r, tp) for r in range(tp)] for n, t in full.items()}
    for n, t in full.items():
        assert sh[n][0].shape == P.local_shape(spec[n], tp, 0) and torch.equal(P.unshard(spec[n], sh[n]), t)
    x = torch.randn(M, D, generator=g0, dtype=torch.float64)
    want = SW.swiglu_fc1(x, full["h.0.fc1.w"], full["h.0.fc1.b"])[1] @ full["h.0.fc2.w"].t()
    got = sum(SW.swiglu_fc1(x, sh["h.0.fc1.w"][r], sh["h.0.fc1.b"][r])[1] @ sh["h.0.fc2.w"][r].t() for r in range(tp))
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_torch_paths_match_float64_autograd():
    g0 = torch.Generator().manual_seed(5)
    M, D, F = 7, 12, 8
    x, w, w2, dy = (torch.randn(s, generator=g0, dtype=torch.float64) for s in ((M, D), (2 * F, D), (D, F), (M, D)))
    b = torch.randn(2 * F, generator=g0, dtype=torch.float64)
    gu_ref = (x @ w.t() + b).requires_grad_(True)
    g, u = gu_ref.chunk(2, 1)
    h_ref = torch.nn.functional.silu(g) * u
    (h_ref @ w2.t()).backward(dy)
    gu, h = SW.swiglu_fc1(x.float(), w.float(), b.float())
    assert torch.allclose(gu.double(), gu_ref, rtol=1e-5, atol=1e-5) and torch.allclose(h.double(), h_ref, rtol=1e-5, atol=1e-5)
    for w2t in (None, w2.t().contiguous().float()):
        dgu = SW.swiglu_fc2_dgrad(dy.float(), w2.float(), w2t, gu_ref.detach().float())
        assert torch.allclose(dgu.double(), gu_ref.grad, rtol=1e-5, atol=1e-5)


def step_vs_oracle(eng, mc, b):
    """One forward + backward of ``eng`` on ``b`` against autograd through the oracle -> (loss, oracle's, worst rel. grad error)."""
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
    worst = max(((eng.flat.g(n).cpu() - params[n].grad).norm() / (params[n].grad.norm() + 1e-12)).item()
                for n in eng.flat.slots)
    return loss, lo.item(), worst


def test_cpu_engine_step_matches_the_oracle():
    eng, mc = _engine()
    assert eng.flat.p("h.0.fc1.w").shape == (2 * mc.d_ff, mc.d_model)
    loss, lo, worst = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    assert abs(loss - lo) < 1e-5 and worst < 1e-4, (loss, lo, worst)  # bounds of tests/test_model_cpu.py


def test_checkpoint_resume_under_the_other_mlp_raises(tmp_path):
    CK.save(_engine()[0], str(tmp_path), 1)
    with pytest.raises(ValueError, match="mlp='swiglu'"):
        CK.load_into(_engine("gelu")[0], str(tmp_path), 1)


@pytest.mark.parametrize("mode", ["fp8", "mxfp8"])
def test_engine_refuses_swiglu_with_the_fp8_forwards(mode):
    with pytest.raises(ValueError, match=f"mlp=swiglu cannot be combined with fwd_gemm_dtype={mode}"):
        _engine(fwd_gemm_dtype=mode)
