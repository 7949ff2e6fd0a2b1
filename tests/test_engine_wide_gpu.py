"""d_model 2048 end to end on the GPU: the gpt-1.3b preset's width and head layout (16 heads of 128) shrunk to
two layers, d_ff 4096, T192 and a 1000-token vocabulary (about 70 M parameters, 384 tokens) against the fp32
autograd oracle in bf16 and in the exact-fp32 mode, and hipGraph replay against eager.  Every LayerNorm of
this model runs the wide backward kernel (d_model > 1024); the forward is the old kernel's widest case."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

BATCH = 2


def _engine(dev, use_graph, **kw):
    mc = model_config_from_preset("gpt-1.3b", vocab_size=1000, n_layers=2, d_ff=4096, max_seq_len=192)
    assert mc.d_model == 2048 and mc.head_dim == 128
    tc = TrainConfig(seed=0, parallel="dp", batch=BATCH, steps=1, log_every=1, output_dir="/tmp/x",
                     use_graph=use_graph, **kw)
    oc = OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, dev, "nccl")), mc


# thresholds: tests/test_engine_hd128_gpu.py (norm-relative per parameter: they do not grow with the width)
@pytest.mark.parametrize("dtype,loss_tol,grad_tol", [("bf16", 2e-2, 5e-2), ("fp32", 1e-4, 1e-3)])
def test_wide_grads_vs_oracle(cuda, dtype, loss_tol, grad_tol):
    eng, mc = _engine(cuda, use_graph=False, **({"dtype": "fp32"} if dtype == "fp32" else {}))
    assert eng.act_dtype == (torch.float32 if dtype == "fp32" else torch.bfloat16)
    b = next(get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999))
    eng.set_batch(b)
    st, T = eng.stage, mc.max_seq_len
    ctx = {}
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    h = st.stage_forward(h, BATCH, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (BATCH * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (BATCH * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    torch.cuda.synchronize()
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
    lo.backward()
    worst = []
    for n in eng.flat.slots:
        g, go = eng.flat.g(n).cpu(), params[n].grad
        worst.append((((g - go).norm() / (go.norm() + 1e-12)).item(), n))
    print(f"wide d2048 {dtype}: loss {loss.item():.6f} oracle {lo.item():.6f}; worst relative grad errors:",
          sorted(worst)[-5:])
    assert abs(loss.item() - lo.item()) < loss_tol, (loss.item(), lo.item())
    for err, n in worst:
        assert err < grad_tol, f"{n}: relative grad error {err:.3e}"


def test_wide_graph_replay_matches_eager(cuda):
    losses = {}
    for mode in (False, True):
        eng, mc = _engine(cuda, use_graph=mode)
        it = get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
        out = []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        losses[mode] = out
        if mode:
            assert eng.program.n_graphs >= 1
    assert losses[True] == pytest.approx(losses[False], rel=1e-5, abs=1e-5), losses
