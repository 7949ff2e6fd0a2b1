"""``OptimConfig.lr_schedule: warmup_cosine`` on the CPU: the host value ``lr_at`` against the optax formula, the
schema refusals, the first (zero-rate) update, resume, and the constant default."""

import math
from dataclasses import replace

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.utils import checkpoint as C

LR, N = 3e-3, 8


def _oc(W=3, r=0.1, **kw):
    return OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0, lr_schedule="warmup_cosine", lr_warmup_steps=W,
                       lr_decay_steps=N, lr_min_ratio=r, **kw)


def _formula(t, W, r):
    """optax.warmup_cosine_decay_schedule(0, lr, W, N, lr * r) at count c = t - 1, in float64."""
    c = t - 1
    if c < W:
        return LR * c / W
    return LR * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * min(c - W, N - W) / (N - W))))


@pytest.mark.parametrize("W", [0, 3])
@pytest.mark.parametrize("r", [0.0, 0.1])
def test_lr_at_matches_formula(W, r):
    oc = _oc(W, r)
    for t in [1, 2, W, W + 1, N, N + 5]:
        if t < 1:
            continue
        assert oc.lr_at(t) == pytest.approx(_formula(t, W, r), rel=1e-15, abs=0.0), (t, W, r)
    if W > 0:
        assert oc.lr_at(1) == 0.0  # optax: the first update is scaled by schedule(0) = 0
    assert oc.lr_at(W + 1) == pytest.approx(LR, rel=1e-15)  # the peak, right after the warmup
    assert oc.lr_at(N + 1) == pytest.approx(LR * r, rel=1e-12, abs=1e-19) and oc.lr_at(N + 50) == oc.lr_at(N + 1)


def test_constant_lr_at():
    oc = OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0)
    assert oc.lr_schedule == "constant" and not oc.scheduled
    assert [oc.lr_at(t) for t in (1, 5, 1000)] == [LR] * 3


@pytest.mark.parametrize("kw", [
    dict(lr_schedule="linear"),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=5, lr_decay_steps=5),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=5, lr_decay_steps=3),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=0, lr_decay_steps=0),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=-1, lr_decay_steps=5),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=1, lr_decay_steps=5, lr_min_ratio=-0.1),
    dict(lr_schedule="warmup_cosine", lr_warmup_steps=1, lr_decay_steps=5, lr_min_ratio=1.5),
    dict(lr_schedule="constant", lr_warmup_steps=-2),
])
def test_schema_refusals(kw):
    with pytest.raises(ValueError):
        OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0, **kw)


def _engine(oc, out="/tmp/unused", **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1000, output_dir=out, device="cpu",
                     warmup_steps=0, dtype="fp32", **kw)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo")), mc


def _steps(eng, mc, it, n):
    for _ in range(n):
        eng.set_batch(next(it))
        eng.run_step()
        eng.loss_value()


def _data(mc):
    return get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)


def test_first_update_has_zero_rate():
    eng, mc = _engine(_oc(W=3))
    p0, m0, v0 = eng.flat.params.clone(), eng.flat.exp_avg.clone(), eng.flat.exp_avg_sq.clone()
    it = _data(mc)
    _steps(eng, mc, it, 1)
    assert eng.opt.lr_value() == 0.0
    assert torch.equal(eng.flat.params, p0), "lr_1 = 0: no parameter may move"
    assert not torch.equal(eng.flat.exp_avg, m0) and not torch.equal(eng.flat.exp_avg_sq, v0)
    _steps(eng, mc, it, 1)
    assert eng.opt.lr_value() == pytest.approx(LR / 3, rel=1e-6)
    assert not torch.equal(eng.flat.params, p0)


def test_device_scalar_follows_schedule_on_cpu():
    oc = _oc(W=3)
    eng, mc = _engine(oc)
    it = _data(mc)
    for t in range(1, 13):
        _steps(eng, mc, it, 1)
        assert eng.opt.lr_value() == pytest.approx(oc.lr_at(t), rel=1e-6, abs=1e-12), t


def test_resume_is_bitwise_and_checks_the_schedule(tmp_path):
    oc = _oc(W=3)
    eng, mc = _engine(oc, out=str(tmp_path))
    it = _data(mc)
    _steps(eng, mc, it, 4)
    C.save(eng, str(tmp_path), 4)
    _steps(eng, mc, it, 2)
    straight = eng.flat.params.clone(), eng.flat.exp_avg.clone(), eng.flat.exp_avg_sq.clone()

    eng2, _ = _engine(oc, out=str(tmp_path))
    C.load_into(eng2, str(tmp_path), 4)
    assert int(eng2.opt.step_t.item()) == 4
    it2 = _data(mc)
    for _ in range(4):
        next(it2)
    _steps(eng2, mc, it2, 2)
    for a, b in zip(straight, (eng2.flat.params, eng2.flat.exp_avg, eng2.flat.exp_avg_sq)):
        assert torch.equal(a, b)

    for other in (replace(oc, lr_warmup_steps=2), replace(oc, lr_min_ratio=0.0), replace(oc, lr_decay_steps=9),
                  OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0)):
        eng3, _ = _engine(other, out=str(tmp_path))
        with pytest.raises(ValueError, match="lr_schedule"):
            C.load_into(eng3, str(tmp_path), 4)


def test_constant_equals_leaving_the_fields_out():
    out = []
    for oc in (OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0),
               OptimConfig(lr=LR, weight_decay=0.1, grad_clip=1.0, lr_schedule="constant")):
        eng, mc = _engine(oc)
        assert eng.opt.sched is None
        _steps(eng, mc, _data(mc), 3)
        out.append(eng.flat.params.clone())
    assert torch.equal(out[0], out[1])
