"""``norm: rmsnorm`` end to end on the GPU (the pattern of tests/test_rope_engine_gpu.py): first-step loss and gradients
against the autograd oracle, then five graph-replayed steps, in bf16, in fp32 and for a bf16 GQA + rope model.  ``wte`` is
shifted by 0.05, about 0.8 of its spread (0.0626): at initialisation the residual rows have almost no mean and the two
norms nearly coincide.  Picked on the CPU from the oracle alone: its ``h.0.qkv.w`` gradient under ``layernorm`` is then
1.03 (1.11 for the GQA + rope model) of its norm away from the one under ``rmsnorm`` (0.84 / 0.94 at a shift of 0.02)."""

import pytest
import torch
from test_rmsnorm_cpu import SHIFT, step_vs_oracle

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

TINY = dict(d_model=256, n_heads=4, n_layers=2, d_ff=512, max_seq_len=128, norm="rmsnorm")
# model, TrainConfig extras, LOSS_TOL, GRAD_TOL of tests/test_rope_engine_gpu.py
CASES = {"bf16": (TINY, {}, 2e-2, 5e-2),
         "fp32": (TINY, dict(dtype="fp32"), 1e-4, 1e-3),
         "bf16_gqa_rope": (dict(TINY, n_kv_heads=2, pos_emb="rope"), {}, 2e-2, 5e-2)}


def _engine(dev, case, batch=4, steps=1, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **CASES[case][0])
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x",
                     **CASES[case][1], **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


@pytest.mark.parametrize("case", list(CASES))
def test_grads_vs_oracle(cuda, case):
    _, _, loss_tol, grad_tol = CASES[case]
    eng, mc = _engine(cuda, case)
    assert "h.0.ln1.b" not in eng.flat.slots and "h.0.ln1.g" in eng.flat.slots
    loss, lo, worst, gap = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)), SHIFT)
    print(f"rmsnorm {case}: loss {loss:.6f} oracle {lo:.6f}; norm gap {gap:.3f}; worst relative grad error {worst:.3e}")
    assert gap >= 10 * grad_tol, f"the oracle's h.0.qkv.w gradient barely depends on the norm ({gap:.3f})"
    assert abs(loss - lo) < loss_tol and worst < grad_tol, (loss, lo, worst)


@pytest.mark.parametrize("case", list(CASES))
def test_five_graph_steps_fall_and_repeat(cuda, case):
    def losses():
        eng, mc = _engine(cuda, case, steps=5, batch=8, use_graph=True)
        it, out = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999), []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        return out, eng.flat.p("h.0.qkv.w").clone()

    (a, pa), (b, pb) = losses(), losses()
    assert a[-1] < a[0] and a == b and torch.equal(pa, pb), (a, b)
