"""``pos_emb: rope`` end to end on the GPU (the pattern of tests/test_gqa_engine_gpu.py): first-step loss and gradients
against the autograd oracle, then five graph-replayed steps, for a bf16 GQA model, the multi-head model in fp32 and under
``doc_mask_token``.  The ``.w`` and ``wte`` parameters are scaled by 2.0 (near-uniform attention would hide a missing
rotation), picked on the CPU from the oracle alone: its ``h.0.qkv.w`` gradient moves by 0.51-0.56 of its norm without
the rotation at 1.0, barely the 10 * GRAD_TOL asked for, and by more than its norm at 2.0 (asserted below)."""

import numpy as np
import pytest
import torch
from test_rope_cpu import step_vs_oracle

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

MHA = dict(d_model=256, n_heads=4, n_layers=2, d_ff=512, max_seq_len=128, pos_emb="rope")
SEP = 7
# model, TrainConfig extras, LOSS_TOL, GRAD_TOL of tests/test_gqa_engine_gpu.py (bf16) / tests/test_engine_gpu.py (fp32)
CASES = {"bf16_gqa": (dict(MHA, n_kv_heads=2), {}, 2e-2, 5e-2),
         "fp32_mha": (MHA, dict(dtype="fp32"), 1e-4, 1e-3),
         "bf16_doc": (MHA, dict(doc_mask_token=SEP), 2e-2, 5e-2)}


def _engine(dev, case, batch=4, steps=1, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **CASES[case][0])
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x",
                     **CASES[case][1], **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


def _batches(mc, n, rows, doc):
    it = get_batch_iterator(rows, mc.max_seq_len + 1, vocab=999)
    out, g = [next(it).copy() for _ in range(n)], np.random.default_rng(11)
    for b in out if doc else ():  # as tests/test_attn_doc_engine_gpu.py: a separator at about every 7th position
        b[g.random(b.shape) < 0.15] = SEP
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_grads_vs_oracle(cuda, case):
    _, extra, loss_tol, grad_tol = CASES[case]
    doc = extra.get("doc_mask_token", -1)
    eng, mc = _engine(cuda, case)
    loss, lo, worst, gap = step_vs_oracle(eng, mc, _batches(mc, 1, 4, doc >= 0)[0], 2.0, doc)
    print(f"rope {case}: loss {loss:.6f} oracle {lo:.6f}; rotation gap {gap:.3f}; worst relative grad error {worst:.3e}")
    assert gap >= 10 * grad_tol, f"the oracle's h.0.qkv.w gradient barely depends on the rotation ({gap:.3f})"
    assert abs(loss - lo) < loss_tol and worst < grad_tol, (loss, lo, worst)


@pytest.mark.parametrize("case", list(CASES))
def test_five_graph_steps_fall_and_repeat(cuda, case):
    def losses():
        eng, mc = _engine(cuda, case, steps=5, batch=8, use_graph=True)
        assert "wpe" not in eng.flat.slots
        out = []
        for b in _batches(mc, 5, 8, "doc" in case):
            eng.set_batch(b)
            eng.run_step()
            out.append(eng.loss_value())
        return out, eng.flat.p("h.0.qkv.w").clone()

    (a, pa), (b, pb) = losses(), losses()
    assert a[-1] < a[0] and a == b and torch.equal(pa, pb), (a, b)
