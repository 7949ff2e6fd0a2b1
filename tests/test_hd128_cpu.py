"""head_dim 128 without a GPU: the small hd-128 model of tests/test_engine_hd128_gpu.py on the torch path: one
engine step against the oracle, and head sharding at head_dim 128 under tp = 2 (gloo) against the single-process
run."""

import pytest
import torch

from test_parallel_cpu import _run

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

SMALL = dict(d_model=256, n_heads=2, d_ff=1024, max_seq_len=192, dropout=0.1)  # 2 layers, head_dim 128


def test_small_hd128_cpu_step_matches_oracle():
    mc = model_config_from_preset("tiny", vocab_size=1000, **SMALL)
    assert mc.head_dim == 128 and mc.n_layers == 2
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/x", device="cpu")
    oc = OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0)
    eng = Engine(mc, tc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"))
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    p0 = {n: eng.flat.p(n).detach().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    lo = oracle_loss(mc, p0, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
    assert abs(eng.loss_value() - lo.item()) < 1e-5, (eng.loss_value(), lo.item())


@pytest.mark.slow
def test_small_hd128_tp2_matches_single_process():
    """One head of 128 per tensor-parallel rank; the tolerance is test_parallel_cpu's for tp 2."""
    model = dict(SMALL, n_layers=2)
    single = _run("dp", 1, model=model)
    res = _run("tp", 2, model=model, tp_sequence_parallel=False)
    assert res[0]["mesh"][1] == 2
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=1e-4, abs=1e-4)
