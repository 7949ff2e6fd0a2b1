"""``TrainConfig.fwd_gemm_dtype: fp8`` on the CPU path: schema, refused settings, the explicit forward / backward
against the fake-quant oracle, and the FP8 weight mirror's freshness."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import (OptimConfig, TrainConfig, build_configs,
                                                                model_config_from_preset)
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.gpt import GPTStage, StageLayout
from distributed_training_compare_jax_amd.models.params import all_param_specs
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import fp8 as F
from distributed_training_compare_jax_amd.parallel.buffers import FlatParams
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.train.loop import train
from distributed_training_compare_jax_amd.utils import checkpoint as C

OC = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0)
CPU = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")
SEED = 0  # chosen with the oracle alone: see test_explicit_backward_matches_fake_quant_oracle


def _mc(**kw):
    d = dict(d_model=128, n_layers=2, n_heads=2, d_ff=512, max_seq_len=64)
    d.update(kw)
    return model_config_from_preset("tiny", vocab_size=1000, **d)


def _tc(out, steps=1, **kw):
    d = dict(seed=0, parallel="dp", batch=4, steps=steps, log_every=1000, output_dir=out, device="cpu",
             warmup_steps=0, fwd_gemm_dtype="fp8")
    d.update(kw)
    return TrainConfig(**d)


# ------------------------------------------------------------------------------------------------- schema

def test_key_loads_from_yaml(tmp_path):
    (tmp_path / "t.yaml").write_text("seed: 0\nparallel: dp\nbatch: 4\nsteps: 1\nlog_every: 1\noutput_dir: o\n"
                                     "fwd_gemm_dtype: fp8\n")
    tc, _, _ = build_configs(str(tmp_path / "t.yaml"))
    assert tc.fwd_gemm_dtype == "fp8"
    assert TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="o").fwd_gemm_dtype == "bf16"


@pytest.mark.parametrize("mc,kw,dinfo,names", [
    (_mc(), dict(dtype="fp32"), CPU, "dtype=fp32"),
    (_mc(), dict(parallel="tp", tp=2), DistInfo(0, 2, 0, torch.device("cpu"), "gloo"), "tp=2"),
    (_mc(), dict(defer_optimizer=True), CPU, "defer_optimizer"),
    (_mc(d_model=64, d_ff=512), {}, CPU, "d_model=64"),
    (_mc(d_ff=320), {}, CPU, "d_ff=320"),
    (_mc(), dict(fwd_gemm_dtype="fp4"), CPU, "fwd_gemm_dtype='fp4'"),
], ids=["fp32", "tp", "defer_optimizer", "d_model", "d_ff", "unknown"])
def test_engine_refuses_what_fp8_does_not_cover(mc, kw, dinfo, names):
    with pytest.raises(ValueError, match=names) as e:
        Engine(mc, _tc("/tmp/unused", **kw), OC, dinfo)
    assert "fwd_gemm_dtype" in str(e.value)


# ----------------------------------------------------------------------------------- forward / backward

def _ulp_neighbours(x):
    return torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, float("-inf")))


def test_explicit_backward_matches_fake_quant_oracle():
    """tests/test_model_cpu.py::test_explicit_backward_matches_autograd with the FP8 forward on both sides.

    Engine and oracle sum in different orders, so a quantiser input on a rounding boundary could flip a byte.
    The seed is the first one for which, with the oracle alone, moving every quantiser input by one fp32 ulp,
    either way, changes no quantised byte and no scale (asserted first).

    One case, dropout 0: dropout acts on the embedding output only, so it adds nothing to what the FP8 path is
    checked on, while the one-ulp rule does not protect the comparison in general: the engine's attention output
    differs from the oracle's softmax by tens of ulps (34 at the first differing byte with dropout 0.1 and seed 1,
    the first seed that passes the rule there), one flipped byte changes the loss by 7.9e-5 against the 1e-5
    tolerance, and with 32k to 131k elements per quantised tensor no seed keeps every element that far from a
    boundary.  The GPU test (tests/test_fp8_engine_gpu.py) bounds that effect with the oracle's own bf16-input
    run instead."""
    dropout = 0.0
    mc = _mc(dropout=dropout)
    specs = all_param_specs(mc)
    flat = FlatParams(specs, 0, 1, "cpu", compute_dtype=torch.float32)
    flat.init_canonical(SEED)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    params = {n: flat.p(n).clone().requires_grad_(True) for n in flat.slots}
    seen = []
    lo = oracle_loss(mc, params, ids, lab, 5, 3, fake_quant=True, quant_inputs=seen)
    lo.backward()
    assert len(seen) == 4 * mc.n_layers
    for i, x in enumerate(seen):
        q = F.quant_e4m3(x)
        for y in _ulp_neighbours(x):
            qy = F.quant_e4m3(y)
            assert torch.equal(q.scale, qy.scale) and torch.equal(q.q, qy.q), \
                f"quantiser input {i}: {int((q.q != qy.q).sum())} bytes change under a one-ulp move"

    st = GPTStage(mc, flat, StageLayout(range(mc.n_layers), True, True), act_dtype=torch.float32, dropout_seed=5)
    st.enable_fp8_forward()
    step = torch.tensor([3])
    ctx = {}
    T = mc.max_seq_len
    h = st.embed_forward(ids, step, 0, ctx)
    h = st.stage_forward(h, 4, ctx)
    loss = st.head_forward(h, lab, 1 / (4 * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (4 * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    st.embed_backward(ctx, dx, step, 0.0)
    assert abs(loss.item() - lo.item()) < 1e-5
    for n in flat.slots:
        assert torch.allclose(flat.g(n), params[n].grad, rtol=1e-4, atol=1e-6), n
    assert not ctx
    # and the FP8 forward is not the plain one
    plain = oracle_loss(mc, {n: flat.p(n) for n in flat.slots}, ids, lab, 5, 3)
    assert abs(plain.item() - lo.item()) > 1e-5


def test_oracle_default_is_unchanged_and_bf16_option_rounds_inputs():
    mc = _mc(dropout=0.0)
    flat = FlatParams(all_param_specs(mc), 0, 1, "cpu", compute_dtype=torch.float32)
    flat.init_canonical(SEED)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    params = {n: flat.p(n) for n in flat.slots}
    a = oracle_loss(mc, params, ids, lab, 5, 3)
    assert torch.equal(a, oracle_loss(mc, params, ids, lab, 5, 3, fake_quant=False))
    seen = []
    oracle_loss(mc, params, ids, lab, 5, 3, fake_quant=True, quant_bf16_inputs=True, quant_inputs=seen)
    assert all(torch.equal(x, x.to(torch.bfloat16).float()) for x in seen)


# ---------------------------------------------------------------------------------------- weight mirror

def _mirror_is_fresh(eng):
    f = eng.flat
    names = [f"h.{l}.{n}.w" for l in range(eng.mcfg.n_layers) for n in ("qkv", "out", "fc1", "fc2")]
    assert sorted(f.mirror_fp8) == sorted(names)
    for n in names:
        want = F.quant_e4m3(f.p(n).to(torch.bfloat16))
        got = f.w8(n)
        assert torch.equal(got.q, want.q) and torch.equal(got.scale, want.scale) and torch.equal(got.inv, want.inv), n


def test_weight_mirror_follows_the_optimizer_and_a_checkpoint(tmp_path):
    mc = _mc()
    r = train(_tc(str(tmp_path / "a"), 2, ckpt_every=2), mc, OC, CPU, quiet=True)
    eng = r["engine"]
    _mirror_is_fresh(eng)
    fresh = Engine(mc, _tc(str(tmp_path / "a"), 2), OC, CPU)
    before = {n: t.q.clone() for n, (_, t) in fresh.flat.mirror_fp8.items()}
    _mirror_is_fresh(fresh)  # at init
    C.load_into(fresh, str(tmp_path / "a"), 2)
    _mirror_is_fresh(fresh)
    assert any(not torch.equal(before[n], t.q) for n, (_, t) in fresh.flat.mirror_fp8.items())
    for n, (_, t) in fresh.flat.mirror_fp8.items():
        assert torch.equal(t.q, eng.flat.w8(n).q)
    assert not any("fp8" in k for k in eng.flat.state_dict())  # not part of a checkpoint
