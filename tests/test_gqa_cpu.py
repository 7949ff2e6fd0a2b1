"""Grouped-query attention without a GPU: ``ModelConfig.n_kv_heads`` in the schema, the parameter inventory and its
tensor-parallel sharding, one engine step on the torch path against the autograd oracle, the engine's refusals."""

import os

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import (ModelConfig, OptimConfig, TrainConfig, load_yaml,
                                                                 model_config_from_preset)
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models import params as P
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(d_model=256, n_heads=4, n_kv_heads=2, d_ff=512, max_seq_len=64, dropout=0.1)  # 2 layers, head_dim 64


def _engine(mc, device="cpu", world=1, **kw):
    tc = TrainConfig(**{**dict(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/x", device=device),
                        **kw})
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                  DistInfo(0, world, 0, torch.device(device), "gloo"))


@pytest.mark.parametrize("kv", [0, 3, 8, True, 2.0])
def test_schema_refuses_what_is_no_divisor(kv):
    with pytest.raises(ValueError, match="n_kv_heads"):
        model_config_from_preset("tiny", n_heads=4, d_model=64, n_kv_heads=kv)


def test_schema_shapes_and_counts():
    mha = model_config_from_preset("tiny", vocab_size=1000, **dict(SMALL, n_kv_heads=None))
    same = model_config_from_preset("tiny", vocab_size=1000, **dict(SMALL, n_kv_heads=4))
    gqa = model_config_from_preset("tiny", vocab_size=1000, **SMALL)
    assert (mha.kv_heads, mha.qkv_rows, same.qkv_rows, gqa.kv_heads, gqa.qkv_rows) == (4, 768, 768, 2, 512)
    assert same.num_params() == mha.num_params() and same.flops_per_token() == mha.flops_per_token()
    # two K/V heads of 64 fewer: per layer 256 weight rows of 256 and 256 biases, 6 matmul FLOPs per weight
    assert mha.num_params() - gqa.num_params() == 2 * (256 * 256 + 256)
    assert mha.flops_per_token() - gqa.flops_per_token() == 6.0 * 2 * 256 * 256
    specs = {s.name: s for s in P.all_param_specs(gqa)}
    assert specs["h.0.qkv.w"].shape == (512, 256) and specs["h.1.qkv.b"].shape == (512,)
    assert sum(int(torch.Size(s.shape).numel()) for s in specs.values()) == gqa.num_params() + (
        gqa.padded_vocab - gqa.vocab_size) * (gqa.d_model + 1)
    assert [s.shape for s in P.all_param_specs(mha)] == [s.shape for s in P.all_param_specs(same)]
    d = load_yaml(os.path.join(ROOT, "configs", "model_config_gpt_1p3b_gqa.yaml"))
    preset = ModelConfig(vocab_size=1000, **d)
    assert (preset.n_heads, preset.kv_heads, preset.head_dim, preset.qkv_rows) == (16, 4, 128, 3072)


def test_tp2_shards_whole_groups_and_round_trips():
    gqa = model_config_from_preset("tiny", vocab_size=1000, **SMALL)
    spec = {s.name: s for s in P.layer_param_specs(gqa, 0)}["h.0.qkv.w"]
    full = torch.arange(512 * 256, dtype=torch.float32).view(512, 256)
    shards = [P.shard(spec, full, r, 2) for r in range(2)]
    for r, s in enumerate(shards):  # rank r: query heads 2r, 2r + 1 and K/V head r, 64 rows each
        assert tuple(s.shape) == P.local_shape(spec, 2, r) == (256, 256)
        want = torch.cat([full[128 * r:128 * r + 128], full[256 + 64 * r:320 + 64 * r], full[384 + 64 * r:448 + 64 * r]])
        assert torch.equal(s, want)
    assert torch.equal(P.unshard(spec, shards), full)
    with pytest.raises(ValueError, match="n_kv_heads 2 is not a multiple of tp 4"):
        P.shard(spec, full, 0, 4)


def test_cpu_step_matches_oracle():
    mc = model_config_from_preset("tiny", vocab_size=1000, **SMALL)
    eng = _engine(mc)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    p0 = {n: eng.flat.p(n).detach().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    lo = oracle_loss(mc, p0, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
    assert abs(eng.loss_value() - lo.item()) < 1e-5, (eng.loss_value(), lo.item())


@pytest.mark.parametrize("kw,why", [(dict(doc_mask_token=7), "doc_mask_token=7"),
                                    (dict(fwd_gemm_dtype="fp8"), "fwd_gemm_dtype=fp8"),
                                    (dict(parallel="tp", tp=4, world=4), "tp=4")])  # refused before any collective
def test_engine_refusals(kw, why):
    mc = model_config_from_preset("tiny", vocab_size=1000, **SMALL)
    with pytest.raises(ValueError, match=f"n_kv_heads=2 cannot be combined with {why}"):
        _engine(mc, **kw)


def test_resume_under_another_value_is_refused(tmp_path):
    from distributed_training_compare_jax_amd.utils import checkpoint as C

    C.save(_engine(model_config_from_preset("tiny", vocab_size=1000, **SMALL)), str(tmp_path), 1)
    other = _engine(model_config_from_preset("tiny", vocab_size=1000, **dict(SMALL, n_kv_heads=1)))
    with pytest.raises(ValueError, match="n_kv_heads=2, this run has n_kv_heads=1"):
        C.source_rank(other, C._read_metas(C._dir(str(tmp_path), 1)))
