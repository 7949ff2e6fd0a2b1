"""``mlp: swiglu`` end to end on the GPU (the pattern of tests/test_rmsnorm_engine_gpu.py): first-step loss and gradients
against the oracle, then five graph-replayed steps; bf16 (fused kernels), fp32 (elementwise), bf16 GQA + rope + RMSNorm."""

import pytest
import torch
from test_swiglu_cpu import step_vs_oracle

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.ops import swiglu as SW
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

TINY = dict(d_model=256, n_heads=4, n_layers=2, d_ff=512, max_seq_len=128, mlp="swiglu")
# model, TrainConfig extras, LOSS_TOL, GRAD_TOL of tests/test_rmsnorm_engine_gpu.py, the path ops/swiglu.py records
CASES = {"bf16": (TINY, {}, 2e-2, 5e-2, "fused"),
         "fp32": (TINY, dict(dtype="fp32"), 1e-4, 1e-3, "unfused"),
         "bf16_gqa_rope_rms": (dict(TINY, n_kv_heads=2, pos_emb="rope", norm="rmsnorm"), {}, 2e-2, 5e-2, "fused")}


def _engine(dev, case, batch=4, steps=1, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **CASES[case][0])
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x",
                     **CASES[case][1], **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


@pytest.mark.parametrize("case", list(CASES))
def test_grads_vs_oracle(cuda, case):
    _, _, loss_tol, grad_tol, path = CASES[case]
    eng, mc = _engine(cuda, case)
    loss, lo, worst = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    print(f"swiglu {case}: loss {loss:.6f} oracle {lo:.6f}; worst relative grad error {worst:.3e}; {SW.LAST}")
    assert SW.LAST == {"fc1": path, "fc2_dgrad": path}
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
        return out, eng.flat.p("h.0.fc1.w").clone()

    (a, pa), (b, pb) = losses(), losses()
    assert a[-1] < a[0] and a == b and torch.equal(pa, pb), (a, b)
