"""The gpt-1.3b preset without a GPU: its fields, its YAML twin, its parameter count from the parameter specs,
and one torch-path engine step of a shrunk wide model (d_model 1280, past the old LayerNorm backward limit,
10 heads of 128) against the oracle."""

import dataclasses
import math
import os

import torch

from distributed_training_compare_jax_amd.config.schema import (MODEL_PRESETS, REFERENCE_VOCAB_SIZE, ModelConfig,
                                                                OptimConfig, TrainConfig, load_yaml,
                                                                model_config_from_preset)
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.params import all_param_specs
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preset_fields():
    assert MODEL_PRESETS["gpt-1.3b"] == dict(d_model=2048, n_layers=24, n_heads=16, d_ff=8192, max_seq_len=2048,
                                             dropout=0.1, name="gpt-1.3b")
    mc = model_config_from_preset("gpt-1.3b")
    assert mc.vocab_size == REFERENCE_VOCAB_SIZE and mc.head_dim == 128


def test_yaml_matches_preset():
    d = load_yaml(os.path.join(ROOT, "configs", "model_config_gpt_1p3b.yaml"))
    assert d == MODEL_PRESETS["gpt-1.3b"]
    names = {f.name for f in dataclasses.fields(ModelConfig)}
    assert set(d) <= names
    assert ModelConfig(vocab_size=REFERENCE_VOCAB_SIZE, **d) == model_config_from_preset("gpt-1.3b")


def test_parameter_count_from_specs():
    mc = model_config_from_preset("gpt-1.3b")
    n = sum(math.prod(s.shape) for s in all_param_specs(mc))
    assert 1.2e9 < n < 1.5e9, n


def test_shrunk_wide_cpu_step_matches_oracle():
    mc = model_config_from_preset("gpt-1.3b", vocab_size=1000, d_model=1280, n_heads=10, n_layers=2, d_ff=1280,
                                  max_seq_len=64)
    assert mc.head_dim == 128 and mc.d_model > 1024
    tc = TrainConfig(seed=0, parallel="dp", batch=2, steps=1, log_every=1, output_dir="/tmp/x", device="cpu")
    oc = OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0)
    eng = Engine(mc, tc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"))
    b = next(get_batch_iterator(2, mc.max_seq_len + 1, vocab=999))
    p0 = {n: eng.flat.p(n).detach().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    lo = oracle_loss(mc, p0, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
    assert abs(eng.loss_value() - lo.item()) < 1e-5, (eng.loss_value(), lo.item())
