"""Rotary embeddings on the CPU: table, torch path of ``rope_`` against float64 at the derived bound (docs/NUMERICS.md
"RoPE"), the relative-position property, the config fields, one engine step against ``models/reference.py``."""

import dataclasses

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops.rope import rope_, rope_table
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine


def amplitudes(shape, dtype, seed=0):
    """Amplitudes 10^U(-2, 2): a bound relative to the maximum would hide the small elements."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 4 - 2)).to(dtype)


def rotate64(x, tab, n_rot, inverse=False):
    """(float64 rotation of the first n_rot heads of x [B, T, .], |lo| + |hi| per rotated element), on the CPU."""
    (B, T, _), hd = x.shape, 2 * tab.shape[1]
    c, s = (tab[:T, :, i].double().cpu()[None, :, None] for i in (0, 1))
    s = -s if inverse else s
    out = x.double().cpu().clone()
    rot = out[..., :n_rot * hd].reshape(B, T, n_rot, 2, hd // 2)
    lo, hi = rot[..., 0, :], rot[..., 1, :]
    mag = torch.zeros_like(out)
    mag[..., :n_rot * hd] = (lo.abs() + hi.abs())[..., None, :].expand_as(rot).reshape(B, T, -1)
    out[..., :n_rot * hd] = torch.stack([lo * c - hi * s, hi * c + lo * s], -2).reshape(B, T, -1)
    return out, mag


def bound(ref, mag, dtype):
    return (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0) + 2.0 ** -20 * mag


@pytest.mark.parametrize("hd,theta", [(32, 10000.0), (128, 500000.0)])
def test_table_against_numpy_float64(hd, theta):
    tab = rope_table(2048, hd, theta).numpy()
    ang = np.arange(2048, dtype=np.float64)[:, None] * theta ** (-2.0 * np.arange(hd // 2, dtype=np.float64) / hd)
    for k, want in enumerate((np.cos(ang), np.sin(ang))):
        assert (np.abs(tab[..., k] - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,Hkv,hd", [(4, 2, 32), (3, 1, 64), (5, 5, 16)])
def test_torch_path_matches_float64(H, Hkv, hd, dtype):
    x, tab, n = amplitudes((2, 37, (H + 2 * Hkv) * hd), dtype), rope_table(40, hd), (H + Hkv) * hd
    for inverse in (False, True):
        y = rope_(x.clone(), tab, H, Hkv, inverse=inverse)
        ref, mag = rotate64(x, tab, H + Hkv, inverse)
        assert ((y.double() - ref).abs() <= bound(ref, mag, dtype)).all()
        assert torch.equal(y[..., n:], x[..., n:]) and torch.equal(y[:, 0], x[:, 0])
    for h, kv, T in ((3, 2, 4), (4, 0, 4), (H, Hkv, 41)):  # H % Hkv, no K/V heads, T beyond the table
        with pytest.raises(ValueError):
            rope_(torch.zeros(1, T, (h + 2 * kv) * hd), tab, h, kv)


def test_scores_depend_on_the_position_difference_only():
    hd, T, shift = 64, 40, 7
    tab = rope_table(T + shift, hd)
    q, k = (amplitudes((1, 1, hd), torch.float64, seed).expand(1, T + shift, hd) for seed in (1, 2))
    rq, rk = rotate64(q, tab, 1)[0][0], rotate64(k, tab, 1)[0][0]  # q and k placed at every position
    s = rq @ rk.t()
    # the fp32 table's entries are within 2^-25 of their angle's; a score is bilinear in two (cos, sin) pairs: 8 x that
    assert (s[:T, :T] - s[shift:, shift:]).abs().max() < 2.0 ** -22 * q[0, 0].norm() * k[0, 0].norm()
    assert (s[0, 1] - s[0, 2]).abs() > 1e-3 * s[0, 1].abs()  # and they do depend on the difference


def test_config_validation_and_num_params():
    mc = model_config_from_preset("tiny", vocab_size=100)
    assert mc.pos_emb == "learned" and mc.rope_theta == 10000.0
    assert mc.num_params() - dataclasses.replace(mc, pos_emb="rope").num_params() == mc.max_seq_len * mc.d_model
    for bad in (dict(pos_emb="alibi"), dict(rope_theta=0.0), dict(rope_theta=float("nan")), dict(rope_theta="1e4"),
                dict(pos_emb="rope", d_model=66, n_heads=2)):  # head_dim 33
        with pytest.raises(ValueError, match="pos_emb|rope_theta"):
            dataclasses.replace(mc, **bad)


def step_vs_oracle(eng, mc, b, scale, doc=-1):
    """One forward + backward of ``eng`` on batch ``b`` with the ``.w`` / ``wte`` parameters scaled (near-uniform
    attention would hide a wrong rotation) against autograd through the oracle -> (loss, oracle loss, worst relative
    gradient error, relative distance of the oracle's h.0.qkv.w gradient to the one with the rotation removed)."""
    for n in eng.flat.slots:
        if n.endswith(".w") or n == "wte":
            eng.flat.p(n).mul_(scale)
    eng.flat.refresh_mirror()
    eng.set_batch(b)
    st, (rows, T), ctx = eng.stage, eng.ids.shape, {}
    eng._doc_bounds_into(ctx, eng.ids)
    h = st.stage_forward(st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx), rows, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (rows * T), ctx).item()
    dx, dxc = st.stage_backward(ctx, *st.head_backward(ctx, 1 / (rows * T), 0.0), 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    lo = oracle_loss(mc, params, ids, lab, 0, 0, doc_mask_token=doc)
    lo.backward()
    flat = dict({n: p.detach().clone().requires_grad_(True) for n, p in params.items()}, wpe=torch.zeros(T, mc.d_model))
    oracle_loss(dataclasses.replace(mc, pos_emb="learned"), flat, ids, lab, 0, 0, doc_mask_token=doc).backward()
    gq = params["h.0.qkv.w"].grad
    worst = max(((eng.flat.g(n).cpu() - params[n].grad).norm() / (params[n].grad.norm() + 1e-12)).item()
                for n in eng.flat.slots)
    return loss, lo.item(), worst, ((gq - flat["h.0.qkv.w"].grad).norm() / gq.norm()).item()


@pytest.mark.parametrize("kv", [None, 2], ids=["mha", "gqa"])
def test_cpu_engine_step_matches_the_oracle(kv):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, n_heads=4, n_kv_heads=kv, pos_emb="rope")
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/unused", device="cpu")
    eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                 DistInfo(0, 1, 0, torch.device("cpu"), "gloo"))
    assert "wpe" not in eng.flat.slots
    # 3.0: at the 6.0 of tests/test_attn_doc_cpu.py the fp32 engine and fp32 autograd are already 7e-5 apart on the
    # learned-table model's gradients (1e-5 at 3.0).  Bounds of tests/test_model_cpu.py
    loss, lo, worst, gap = step_vs_oracle(eng, mc, next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)), 3.0)
    assert gap > 0.5, f"the oracle's h.0.qkv.w gradient barely depends on the rotation ({gap:.3f})"
    assert abs(loss - lo) < 1e-5 and worst < 1e-4, (loss, lo, worst)
