"""``qk_norm: rmsnorm`` end to end on the GPU (tests/test_rope_engine_gpu.py's pattern, shapes and tolerances): first-step
loss and gradients (all, and the gains of every layer on their own) against the autograd oracle, then five graph-replayed
steps run twice; head_dim 64 and 128 in bf16, fp32, and the bf16 GQA + rope + rmsnorm + swiglu block."""

import pytest
import torch
from test_qknorm_cpu import step_vs_oracle

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

TINY = dict(d_model=256, n_heads=4, n_layers=2, d_ff=512, max_seq_len=128, qk_norm="rmsnorm")
CASES = {"bf16_hd64": (TINY, {}, 2e-2, 5e-2),  # model, TrainConfig extras, LOSS_TOL, GRAD_TOL of test_rope_engine_gpu.py
         "bf16_hd128_rope": (dict(TINY, n_heads=2, pos_emb="rope"), {}, 2e-2, 5e-2),
         "fp32_hd64_rope": (dict(TINY, pos_emb="rope"), dict(dtype="fp32"), 1e-4, 1e-3),
         "bf16_gqa_rope_rms_swiglu": (dict(TINY, n_kv_heads=2, pos_emb="rope", norm="rmsnorm", mlp="swiglu"), {}, 2e-2, 5e-2)}


def _engine(dev, case, batch=4, steps=1, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **CASES[case][0])
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x",
                     **CASES[case][1], **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


@pytest.mark.parametrize("case", list(CASES))
def test_grads_vs_oracle(cuda, case):
    _, _, loss_tol, grad_tol = CASES[case]
    eng, mc = _engine(cuda, case)
    assert "h.0.qn.g" in eng.flat.slots and "h.1.kn.g" in eng.flat.slots
    loss, lo, worst, worst_g = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    print(f"qk_norm {case}: loss {loss:.6f} oracle {lo:.6f}; worst relative grad error {worst:.3e}, gains {worst_g:.3e}")
    assert abs(loss - lo) < loss_tol and worst < grad_tol and worst_g < grad_tol, (loss, lo, worst, worst_g)


@pytest.mark.parametrize("case", ["bf16_hd128_rope", "bf16_gqa_rope_rms_swiglu"])
def test_five_graph_steps_fall_and_repeat(cuda, case):
    def losses():
        eng, mc = _engine(cuda, case, steps=5, batch=8, use_graph=True)
        it, out = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999), []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        return out, torch.cat([eng.flat.p("h.0.qkv.w").flatten(), eng.flat.p("h.0.qn.g"), eng.flat.p("h.1.kn.g")])

    (a, pa), (b, pb) = losses(), losses()
    assert a[-1] < a[0] and a == b and torch.equal(pa, pb), (a, b)
