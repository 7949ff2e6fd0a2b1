"""QK-norm without a GPU: ``ModelConfig.qk_norm`` in the schema and the parameter inventory, engine steps on the torch
path of ``ops/qknorm.py`` against the autograd oracle (loss and gradients), the engine's and the checkpoint's refusals."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models import params as P
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine


def _mc(**kw):
    return model_config_from_preset("tiny", vocab_size=1000, **{**dict(qk_norm="rmsnorm"), **kw})


def _engine(mc, device="cpu", world=1, **kw):
    tc = TrainConfig(**{**dict(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/x", device=device), **kw})
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, world, 0, torch.device(device), "gloo"))


def test_schema_and_param_inventory():
    with pytest.raises(ValueError, match="qk_norm='layernorm': expected 'none' or 'rmsnorm'"):
        _mc(qk_norm="layernorm")
    off, on = _mc(qk_norm="none"), _mc(n_heads=4, n_kv_heads=2)
    assert "h.0.qn.g" not in [s.name for s in P.all_param_specs(off)]
    assert on.num_params() - _mc(qk_norm="none", n_heads=4, n_kv_heads=2).num_params() == 2 * on.n_layers * on.head_dim
    specs = P.all_param_specs(on)
    assert sum(int(torch.Size(s.shape).numel()) for s in specs) == on.num_params() + (
        on.padded_vocab - on.vocab_size) * (on.d_model + 1)
    names = [s.name for s in P.layer_param_specs(on, 1)]
    i = names.index("h.1.out.b")
    assert names[i:i + 4] == ["h.1.out.b", "h.1.qn.g", "h.1.kn.g", "h.1.qkv.w"]  # where the backward produces them
    g = {s.name: s for s in specs}["h.0.kn.g"]
    assert (g.shape, g.init, g.tp) == ((on.head_dim,), "ones", "rep")


def _move_gains(eng, mc, gains=(1.5, 0.75)):
    for l in range(2 * mc.n_layers):  # away from their init of ones, so that they are seen to act
        eng.flat.p(f"h.{l // 2}.{('qn.g', 'kn.g')[l % 2]}").mul_(gains[l % 2])


@pytest.mark.parametrize("kw", [dict(), dict(pos_emb="rope"), dict(pos_emb="rope", n_heads=4, n_kv_heads=2)],
                         ids=["learned", "rope", "rope-gqa"])
def test_cpu_step_matches_oracle(kw):
    mc = _mc(**kw)
    eng = _engine(mc)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    _move_gains(eng, mc)
    p0 = {n: eng.flat.p(n).detach().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    lo = oracle_loss(mc, p0, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
    assert abs(eng.loss_value() - lo.item()) < 1e-5, (eng.loss_value(), lo.item())


def step_vs_oracle(eng, mc, b):
    """One forward + backward against autograd through the oracle -> (loss, oracle loss, worst relative grad error, gains')."""
    _move_gains(eng, mc)
    eng.flat.refresh_mirror()
    eng.set_batch(b)
    st, (rows, T), ctx = eng.stage, eng.ids.shape, {}
    h = st.stage_forward(st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx), rows, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (rows * T), ctx).item()
    dx, _ = st.stage_backward(ctx, *st.head_backward(ctx, 1 / (rows * T), 0.0), 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous(), 0, 0)
    lo.backward()
    err = {n: ((eng.flat.g(n).cpu() - params[n].grad).norm() / (params[n].grad.norm() + 1e-12)).item()
           for n in eng.flat.slots}
    return loss, lo.item(), max(err.values()), max(v for n, v in err.items() if n.endswith(("qn.g", "kn.g")))


@pytest.mark.parametrize("kw", [dict(), dict(pos_emb="rope", n_heads=4, n_kv_heads=2, norm="rmsnorm", mlp="swiglu")])
def test_cpu_gradients_match_the_oracle(kw):
    mc = _mc(**kw)
    loss, lo, worst, worst_g = step_vs_oracle(_engine(mc), mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    assert abs(loss - lo) < 1e-5 and worst < 1e-4 and worst_g < 1e-4, (loss, lo, worst, worst_g)  # tests/test_model_cpu.py


@pytest.mark.parametrize("mkw,kw,why", [(dict(), dict(parallel="tp", tp=2, world=2), "tp=2"),
                                        (dict(), dict(fwd_gemm_dtype="fp8"), "fwd_gemm_dtype=fp8"),
                                        (dict(n_heads=4), dict(device="cuda"), "head_dim 16 on the GPU")])
def test_engine_refusals(mkw, kw, why):  # each is refused before any device or collective is touched
    with pytest.raises(ValueError, match=f"qk_norm=rmsnorm cannot be combined with {why}"):
        _engine(_mc(**mkw), **kw)


def test_resume_under_another_value_is_refused(tmp_path):
    from distributed_training_compare_jax_amd.utils import checkpoint as C

    C.save(_engine(_mc(qk_norm="none")), str(tmp_path), 1)
    metas = C._read_metas(C._dir(str(tmp_path), 1))
    assert all(m.pop("qk_norm") == "none" for m in metas.values())  # and a checkpoint from before the field reads as 'none'
    with pytest.raises(ValueError, match="qk_norm='none', this run has qk_norm='rmsnorm'"):
        C.source_rank(_engine(_mc()), metas)
