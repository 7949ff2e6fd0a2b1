"""The MXFP8 quantiser's definition (the torch CPU path of ``ops/mxfp8.py``), the CPU forms of the MXFP8 linears
and fused producers, and ``TrainConfig.fwd_gemm_dtype: mxfp8`` on the CPU path: schema, refused settings and the
explicit forward / backward against the MX fake-quant oracle.

The GPU kernels are held to this path bit for bit in ``tests/test_mxfp8_gpu.py``."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import (OptimConfig, TrainConfig, build_configs,
                                                                model_config_from_preset)
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.gpt import GPTStage, StageLayout
from distributed_training_compare_jax_amd.models.params import all_param_specs
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import gemm as G
from distributed_training_compare_jax_amd.ops import layernorm as LN
from distributed_training_compare_jax_amd.ops import mxfp8 as MX
from distributed_training_compare_jax_amd.parallel.buffers import FlatParams
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.train.loop import train
from distributed_training_compare_jax_amd.utils import checkpoint as C

OC = OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0)
CPU = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")


def _decades(M, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, K, generator=g) * 9 - 6)


def _blocks(x):
    return x.view(x.shape[0], -1, 32)


# --------------------------------------------------------------------------------------------- definition

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_scaled_block_amax_in_range_and_nothing_saturates(dtype):
    x = _decades(37, 256).to(dtype)
    t = MX.quant_mxfp8(x)
    assert t.q.dtype == torch.uint8 and t.q.shape == x.shape and t.sc.dtype == torch.uint8 and t.sc.shape == (37, 8)
    amax = _blocks(x.float()).abs().amax(-1)
    scaled = torch.ldexp(amax, 127 - t.sc.to(torch.int32))
    assert bool((amax > 0).all())
    assert bool(((scaled > 224) & (scaled <= 448)).all()), (scaled.min().item(), scaled.max().item())
    assert int(t.sc.min()) >= 1 and int(t.sc.max()) <= 253
    assert bool(((t.q & 0x7f) != 0x7f).all())  # no NaN code: nothing saturates
    # every block's largest byte is in the top binade pair of e4m3 (224 < |q| <= 448)
    top = _blocks(t.q.view(torch.float8_e4m3fn).float()).abs().amax(-1)
    assert bool(((top >= 224) & (top <= 448)).all())
    # the bytes are the RNE e4m3 of the exactly scaled values
    want = torch.ldexp(_blocks(x.float()), (127 - t.sc.to(torch.int32))[..., None]).to(torch.float8_e4m3fn)
    assert torch.equal(_blocks(t.q), want.view(torch.uint8))


def test_zero_block_gives_scale_127_and_zero_bytes():
    x = _decades(5, 96, seed=1)
    x[2, 32:64] = 0.0
    x[4] = 0.0
    t = MX.quant_mxfp8(x)
    assert int(t.sc[2, 1]) == 127 and bool((t.q[2, 32:64] == 0).all())
    assert bool((t.sc[4] == 127).all()) and bool((t.q[4] == 0).all())
    assert int(t.sc[2, 0]) != 127 or bool((t.q[2, :32] != 0).any())
    assert torch.equal(MX.dequant(t)[4], torch.zeros(96))


def test_requantising_the_dequantised_tensor_is_the_identity():
    """``quant(dequant(quant(x)))`` against ``quant(x)``, every block.  The values are identical everywhere, and
    bytes and scale byte are identical in every block but one kind: the scale rule's interval (224, 448] is
    half-open, so a block whose scaled amax lies in (224, 232] has its largest element rounded DOWN to 224, the one
    e4m3 value outside the interval.  Requantised, that amax (mantissa exactly 1.75) takes the other branch of the
    rule: scale exponent one higher, largest element 448, the same values.  Such blocks are asserted to change in
    exactly that way (scale byte one lower, identical dequantised values), all others to be bitwise equal, and the
    data is asserted to hold both kinds."""
    for seed, dtype in ((2, torch.float32), (3, torch.bfloat16)):
        t = MX.quant_mxfp8(_decades(33, 160, seed=seed).to(dtype))
        d = MX.dequant(t)
        assert d.dtype == torch.float32
        t2 = MX.quant_mxfp8(d)
        assert torch.equal(MX.dequant(t2), d)
        top = _blocks(t.q.view(torch.float8_e4m3fn).float()).abs().amax(-1)
        edge = top == 224.0
        assert 0 < int(edge.sum()) < edge.numel() // 4
        assert torch.equal(t2.sc[~edge], t.sc[~edge]) and torch.equal(_blocks(t2.q)[~edge], _blocks(t.q)[~edge])
        assert torch.equal(t2.sc[edge].to(torch.int32), t.sc[edge].to(torch.int32) - 1)
        top2 = _blocks(t2.q.view(torch.float8_e4m3fn).float()).abs().amax(-1)
        assert bool((top2[edge] == 448.0).all())
        # a third pass changes nothing any more
        t3 = MX.quant_mxfp8(MX.dequant(t2))
        assert torch.equal(t3.q, t2.q) and torch.equal(t3.sc, t2.sc)


@pytest.mark.parametrize("k", [-9, -1, 3, 17])
def test_power_of_two_times_a_block_moves_only_its_scale_byte(k):
    x = torch.randn(6, 128, generator=torch.Generator().manual_seed(4))
    t = MX.quant_mxfp8(x)
    y = x.clone()
    y[3, 64:96] *= 2.0 ** k
    u = MX.quant_mxfp8(y)
    assert torch.equal(u.q, t.q)
    want = t.sc.to(torch.int32)
    want[3, 2] += k
    assert torch.equal(u.sc.to(torch.int32), want)


def test_blocks_are_independent():
    x = _decades(4, 128, seed=5)
    t = MX.quant_mxfp8(x)
    y = x.clone()
    y[1, 32:64] = torch.randn(32, generator=torch.Generator().manual_seed(6)) * 1e4
    u = MX.quant_mxfp8(y)
    same = torch.ones(4, 4, dtype=torch.bool)
    same[1, 1] = False
    assert torch.equal(u.sc[same], t.sc[same])
    assert torch.equal(_blocks(u.q)[same], _blocks(t.q)[same])
    assert int(u.sc[1, 1]) != int(t.sc[1, 1])


def test_scale_rule_at_its_edges():
    """amax a power of two -> scaled amax 256; amax 1.75 * 2^e -> exactly 448; just above -> 224-side exponent."""
    x = torch.zeros(3, 32)
    x[0, 0], x[1, 0], x[2, 0] = -4.0, 1.75, 1.75 * (1 + 2.0 ** -7)  # the last: bf16-exact, just above 448 / 256
    x[:, 1] = 0.3
    t = MX.quant_mxfp8(x)
    scaled = torch.ldexp(x[:, 0].abs(), 127 - t.sc[:, 0].to(torch.int32))
    assert scaled.tolist() == [256.0, 448.0, 224.0 * (1 + 2.0 ** -7)]
    assert t.q[1, 0].item() == 0x7e  # 448, the largest finite e4m3


def test_input_checks():
    with pytest.raises(ValueError):
        MX.quant_mxfp8(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        MX.quant_mxfp8(torch.zeros(4, 64).t())
    with pytest.raises(TypeError):
        MX.quant_mxfp8(torch.zeros(4, 64, dtype=torch.float16))


def test_batched_form_into_preallocated_outputs():
    xs = [_decades(2 + i, 64, seed=10 + i) for i in range(MX.QT_MAX + 2)]
    outs = [MX.MxFp8Tensor(torch.full(x.shape, 0xAA, dtype=torch.uint8), torch.zeros(x.shape[0], 2, dtype=torch.uint8))
            for x in xs]
    got = MX.quant_mxfp8_batch(xs, outs)
    for x, o, g in zip(xs, outs, got):
        w = MX.quant_mxfp8(x)
        assert g.q is o.q and torch.equal(o.q, w.q) and torch.equal(o.sc, w.sc)


# --------------------------------------------------------------------------------------------- CPU linears

def test_cpu_linears_compute_on_dequantised_operands():
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(9, 128, generator=g), torch.randn(32, 128, generator=g) * 0.1
    b, r = torch.randn(32, generator=g), torch.randn(9, 32, generator=g)
    xq, wq = MX.quant_mxfp8(x), MX.quant_mxfp8(w)
    u = MX.dequant(xq) @ MX.dequant(wq).t() + b
    assert torch.equal(MX.linear_mxfp8(xq, wq, b, out_dtype=torch.float32), u)
    assert MX.linear_mxfp8(xq, wq, b).dtype == torch.bfloat16
    out = r.clone()
    assert MX.linear_resid_mxfp8(xq, wq, b, out, out=out) is out and torch.equal(out, u + r)
    d, gl = MX.linear_gelu_mxfp8(xq, wq, b, out_dtype=torch.float32)
    assert torch.equal(gl, G.gelu_tanh(u)) and torch.equal(d, G.gelu_tanh_grad(u))
    d2, g2, gq = MX.linear_gelu_mxfp8(xq, wq, b, out_dtype=torch.float32, quant_out=True)
    w2 = MX.quant_mxfp8(g2)
    assert torch.equal(d2, d) and torch.equal(g2, gl) and torch.equal(gq.q, w2.q) and torch.equal(gq.sc, w2.sc)
    # the block scales matter: the per-tensor view of the same bytes is a different product
    assert (MX.dequant(xq) - x).abs().max() < 2.0 ** -4 * x.abs().max()


def test_cpu_linears_refuse_unsupported_shapes():
    q = lambda r, c: MX.MxFp8Tensor(torch.zeros(r, c, dtype=torch.uint8), torch.full((r, c // 32), 127, dtype=torch.uint8))
    for M, Nn, K in [(4, 32, 64), (4, 24, 128), (4, 32, 192)]:
        for fn in (lambda: MX.linear_mxfp8(q(M, K), q(Nn, K)), lambda: MX.linear_resid_mxfp8(q(M, K), q(Nn, K), None, None),
                   lambda: MX.linear_gelu_mxfp8(q(M, K), q(Nn, K), None)):
            with pytest.raises(NotImplementedError):
                fn()
    with pytest.raises(NotImplementedError):
        MX.linear_gelu_mxfp8(q(4, 128), q(48, 128), None, quant_out=True)  # N % 32 != 0 has no MX form


def test_cpu_layernorm_forms_return_the_quantiser_of_y():
    g = torch.Generator().manual_seed(8)
    x, r = torch.randn(7, 128, generator=g), torch.randn(7, 128, generator=g)
    ga, be = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    (y, mu, rs), yq = MX.layernorm_fwd_mx(x, ga, be, 1e-6)
    y0, mu0, rs0 = LN.layernorm_fwd(x, ga, be, 1e-6)
    w = MX.quant_mxfp8(y0)
    assert torch.equal(y, y0) and torch.equal(mu, mu0) and torch.equal(rs, rs0)
    assert torch.equal(yq.q, w.q) and torch.equal(yq.sc, w.sc)
    for d in (x.clone(), x.to(torch.bfloat16)):
        xs, (y, mu, rs), yq = MX.add_layernorm_fwd_mx(d.clone(), r, ga, be, 1e-6)
        xs0, (y0, mu0, rs0) = LN.add_layernorm_fwd(d.clone(), r, ga, be, 1e-6)
        w = MX.quant_mxfp8(y0)
        assert torch.equal(xs, xs0) and torch.equal(y, y0) and torch.equal(yq.q, w.q) and torch.equal(yq.sc, w.sc)


# ------------------------------------------------------------------------------------------------- schema

def _mc(**kw):
    d = dict(d_model=128, n_layers=2, n_heads=2, d_ff=512, max_seq_len=64)
    d.update(kw)
    return model_config_from_preset("tiny", vocab_size=1000, **d)


def _tc(out, steps=1, **kw):
    d = dict(seed=0, parallel="dp", batch=4, steps=steps, log_every=1000, output_dir=out, device="cpu",
             warmup_steps=0, fwd_gemm_dtype="mxfp8")
    d.update(kw)
    return TrainConfig(**d)


def test_key_loads_from_yaml(tmp_path):
    (tmp_path / "t.yaml").write_text("seed: 0\nparallel: dp\nbatch: 4\nsteps: 1\nlog_every: 1\noutput_dir: o\n"
                                     "fwd_gemm_dtype: mxfp8\n")
    tc, _, _ = build_configs(str(tmp_path / "t.yaml"))
    assert tc.fwd_gemm_dtype == "mxfp8"


@pytest.mark.parametrize("mc,kw,dinfo,names", [
    (_mc(), dict(dtype="fp32"), CPU, "dtype=fp32"),
    (_mc(), dict(parallel="tp", tp=2), DistInfo(0, 2, 0, torch.device("cpu"), "gloo"), "tp=2"),
    (_mc(), dict(defer_optimizer=True), CPU, "defer_optimizer"),
    (_mc(d_model=64, d_ff=512), {}, CPU, "d_model=64"),
    (_mc(d_ff=320), {}, CPU, "d_ff=320"),
], ids=["fp32", "tp", "defer_optimizer", "d_model", "d_ff"])
def test_engine_refuses_what_mxfp8_does_not_cover(mc, kw, dinfo, names):
    with pytest.raises(ValueError, match=names) as e:
        Engine(mc, _tc("/tmp/unused", **kw), OC, dinfo)
    assert "fwd_gemm_dtype=mxfp8" in str(e.value)


def test_other_values_are_still_refused():
    for v in ("fp4", "mxfp4", "e5m2"):
        with pytest.raises(ValueError, match=f"fwd_gemm_dtype='{v}'"):
            Engine(_mc(), _tc("/tmp/unused", fwd_gemm_dtype=v), OC, CPU)


# ----------------------------------------------------------------------------------- forward / backward

def _ulp_neighbours(x):
    return torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, float("-inf")))


def _first_stable_seed(mc, ids, lab, flat_of):
    """The first init seed for which, with the oracle alone, moving every quantiser input by one fp32 ulp, either
    way, changes no quantised byte and no scale byte (engine and oracle sum in different orders; the rule and its
    limits: tests/test_fp8_model_cpu.py)."""
    for seed in range(64):
        flat = flat_of(seed)
        seen = []
        oracle_loss(mc, {n: flat.p(n) for n in flat.slots}, ids, lab, 5, 3, fake_quant="mx", quant_inputs=seen)
        ok = len(seen) == 4 * mc.n_layers
        for x in seen:
            q = MX.quant_mxfp8(x)
            ok = ok and all(torch.equal(q.q, qy.q) and torch.equal(q.sc, qy.sc)
                            for qy in map(MX.quant_mxfp8, _ulp_neighbours(x)))
        if ok:
            return seed, flat
    raise AssertionError("no seed in 0..63 keeps every quantiser input one ulp away from a rounding boundary")


def test_explicit_backward_matches_mx_fake_quant_oracle():
    """One CPU engine forward / backward with the MXFP8 forward against the MX fake-quant oracle, at the tolerances
    of tests/test_fp8_model_cpu.py::test_explicit_backward_matches_fake_quant_oracle (loss 1e-5, gradients rtol 1e-4
    atol 1e-6), dropout 0, on the first seed that passes that test's one-ulp rule for the MX quantiser."""
    mc = _mc(dropout=0.0)
    specs = all_param_specs(mc)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()

    def flat_of(seed):
        f = FlatParams(specs, 0, 1, "cpu", compute_dtype=torch.float32)
        f.init_canonical(seed)
        return f

    seed, flat = _first_stable_seed(mc, ids, lab, flat_of)
    print(f"MXFP8-CPU | init seed {seed}")
    params = {n: flat.p(n).clone().requires_grad_(True) for n in flat.slots}
    lo = oracle_loss(mc, params, ids, lab, 5, 3, fake_quant="mx")
    lo.backward()

    st = GPTStage(mc, flat, StageLayout(range(mc.n_layers), True, True), act_dtype=torch.float32, dropout_seed=5)
    st.enable_mxfp8_forward()
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
    # the MX forward is neither the plain one nor the per-tensor one, and fake_quant=True is what it was
    plain = oracle_loss(mc, {n: flat.p(n) for n in flat.slots}, ids, lab, 5, 3)
    per_tensor = oracle_loss(mc, {n: flat.p(n) for n in flat.slots}, ids, lab, 5, 3, fake_quant=True)
    assert abs(plain.item() - lo.item()) > 1e-5 and per_tensor.item() != lo.item()
    with pytest.raises(ValueError):
        oracle_loss(mc, {n: flat.p(n) for n in flat.slots}, ids, lab, 5, 3, fake_quant="fp4")


# ---------------------------------------------------------------------------------------- weight mirror

def _mirror_is_fresh(eng):
    f = eng.flat
    names = [f"h.{l}.{n}.w" for l in range(eng.mcfg.n_layers) for n in ("qkv", "out", "fc1", "fc2")]
    assert sorted(f.mirror_mx) == sorted(names) and not f.mirror_fp8
    for n in names:
        want = MX.quant_mxfp8(f.p(n).to(torch.bfloat16))
        got = f.wmx(n)
        assert torch.equal(got.q, want.q) and torch.equal(got.sc, want.sc), n


def test_weight_mirror_follows_the_optimizer_and_a_checkpoint(tmp_path):
    mc = _mc()
    r = train(_tc(str(tmp_path / "a"), 2, ckpt_every=2), mc, OC, CPU, quiet=True)
    eng = r["engine"]
    _mirror_is_fresh(eng)
    fresh = Engine(mc, _tc(str(tmp_path / "a"), 2), OC, CPU)
    before = {n: t.q.clone() for n, (_, t) in fresh.flat.mirror_mx.items()}
    _mirror_is_fresh(fresh)  # at init
    C.load_into(fresh, str(tmp_path / "a"), 2)
    _mirror_is_fresh(fresh)
    assert any(not torch.equal(before[n], t.q) for n, (_, t) in fresh.flat.mirror_mx.items())
    assert not any("mx" in k for k in eng.flat.state_dict())  # not part of a checkpoint
