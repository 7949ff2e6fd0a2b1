"""``ModelConfig.n_kv_heads`` end to end on the GPU: one small model (4 query heads and 2 K/V heads of 64, two layers,
T 128) against the autograd oracle with repeated K/V heads at the tolerances tests/test_engine_gpu.py uses for the
multi-head model, then five steps: the loss falls and two runs give the same bits."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

MODEL = dict(d_model=256, n_heads=4, n_kv_heads=2, n_layers=2, d_ff=512, max_seq_len=128)
LOSS_TOL, GRAD_TOL = 2e-2, 5e-2  # tests/test_engine_gpu.py test_model_grads_vs_oracle (bf16)


def _engine(dev, batch=4, steps=1, model=MODEL, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **model)
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x", **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


def test_grads_vs_oracle(cuda):
    eng, mc = _engine(cuda)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    eng.set_batch(b)
    st, T = eng.stage, mc.max_seq_len
    ctx = {}
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    h = st.stage_forward(h, 4, ctx)
    assert A.last_launch().path == "fwd_rows32_gqa", A.last_launch()
    loss = st.head_forward(h, eng.labels, 1 / (4 * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (4 * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    assert A.last_launch().path == "bwd_rows32_gqa_merged", A.last_launch()
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    torch.cuda.synchronize()
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous(), 0, 0)
    lo.backward()
    worst = sorted((((eng.flat.g(n).cpu() - params[n].grad).norm() / (params[n].grad.norm() + 1e-12)).item(), n)
                   for n in eng.flat.slots)
    assert abs(loss.item() - lo.item()) < LOSS_TOL, (loss.item(), lo.item())
    for err, n in worst:
        assert err < GRAD_TOL, f"{n}: relative grad error {err:.3e}"


def test_five_steps_fall_and_repeat(cuda):
    def losses():
        eng, mc = _engine(cuda, steps=5, batch=8, use_graph=True)
        it = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999)
        out = []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        return out, eng.flat.p("h.0.qkv.w").clone()

    (a, pa), (b, pb) = losses(), losses()
    assert a[-1] < a[0], a
    assert a == b and torch.equal(pa, pb), "two runs differ"


@pytest.mark.parametrize("kw,why", [(dict(dtype="fp32"), "dtype=fp32 on the GPU"),
                                    (dict(model=dict(MODEL, d_model=128)), "head_dim 32 on the GPU")])
def test_gpu_refusals(cuda, kw, why):
    with pytest.raises(ValueError, match=f"n_kv_heads=2 cannot be combined with {why}"):
        _engine(cuda, **kw)
