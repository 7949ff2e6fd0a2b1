"""``fwd_gemm_dtype: mxfp8`` in the engine on the GPU: mirror freshness (C1), wiring in situ (C2), loss and gradients
against the MX fake-quant oracle (C3), graph replay / determinism / launch record / fusion changes no byte (C4),
training (C5), the wide-LayerNorm fallback (C6).

Small model: d_model 128, 2 layers, 2 heads (head_dim 64), d_ff 512, T 128, vocab 1000, batch 4."""

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import mxfp8 as MX
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

from test_mxfp8_gpu import EPS_BF16, MARGIN, _floor  # this suite's own helpers (tests/test_mxfp8_gpu.py)

pytestmark = pytest.mark.gpu
DENSE = ("qkv", "out", "fc1", "fc2")


def _engine(dev, use_graph=True, dropout=0.1, fwd="mxfp8", lr=1e-3, mc_kw=None, batch=4, **kw):
    d = dict(d_model=128, n_layers=2, n_heads=2, d_ff=512, max_seq_len=128, dropout=dropout)
    d.update(mc_kw or {})
    mc = model_config_from_preset("tiny", vocab_size=1000, **d)
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=1, log_every=1, output_dir="/tmp/x", use_graph=use_graph,
                     fwd_gemm_dtype=fwd, **kw)
    return Engine(mc, tc, OptimConfig(lr=lr, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


def _steps(eng, mc, n, batch=4):
    it = get_batch_iterator(batch, mc.max_seq_len + 1, vocab=999)
    out = []
    for _ in range(n):
        eng.set_batch(next(it))
        eng.run_step()
        out.append(eng.loss_value())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_weight_mirror_is_fresh_after_steps(cuda, use_graph):
    """C1: after two steps each MXFP8 weight copy equals the GPU quantiser's output on the bf16 mirror, bitwise."""
    eng, mc = _engine(cuda, use_graph=use_graph)
    before = {n: (t.q.clone(), t.sc.clone()) for n, (_, t) in eng.flat.mirror_mx.items()}
    _steps(eng, mc, 2)
    assert sorted(eng.flat.mirror_mx) == sorted(f"h.{l}.{n}.w" for l in range(2) for n in DENSE)
    assert not eng.flat.mirror_fp8
    for n, (_, t) in eng.flat.mirror_mx.items():
        want = MX.quant_mxfp8(eng.flat.w(n).contiguous())
        assert torch.equal(t.q, want.q) and torch.equal(t.sc, want.sc), n
        assert not torch.equal(t.q, before[n][0]), f"{n}: the mirror did not move in two steps"


def test_forward_wiring_in_situ(cuda):
    """C2: after one forward each layer's qkv, gelu'(u) and gelu(u) in ctx sit within the bf16 floor bound of a
    float64 reference built from ctx's own inputs (y1, y2) and the bf16 mirror weight, both quantised by the CPU
    path: a stale mirror, a swapped scale tensor or the wrong input fails it."""
    from distributed_training_compare_jax_amd.ops import gemm as G

    eng, mc = _engine(cuda, use_graph=False)
    eng.set_batch(next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    st, ctx = eng.stage, {}
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    st.stage_forward(h, 4, ctx)
    torch.cuda.synchronize()
    ll = MX.last_launch_mxfp8()
    assert ll.variant == "mxfp8_64x128"
    for l in range(mc.n_layers):
        x, y1, mu1, rs1, qkv, o, lse, x2, y2, mu2, rs2, u, gact, batch = ctx[l]

        def ref(inp, name):
            a = MX.dequant(MX.quant_mxfp8(inp.cpu())).double()
            w = MX.dequant(MX.quant_mxfp8(eng.flat.w(f"h.{l}.{name}.w").cpu().contiguous())).double()
            acc = a @ w.t() + eng.flat.p(f"h.{l}.{name}.b").double().cpu()
            return acc, a.abs() @ w.abs().t(), MARGIN * _floor(a[:96], w[:80])

        acc, d, t = ref(y1, "qkv")
        err = (qkv.double().cpu() - acc).abs()
        assert bool((err <= EPS_BF16 * acc.abs() + t * d + 1e-30).all()), f"layer {l} qkv: {(err / d).max().item():.3e}"
        acc, d, t = ref(y2, "fc1")
        v = acc.clone().requires_grad_(True)
        dg = G.gelu_tanh_grad(v)
        (ddg,) = torch.autograd.grad(dg.sum(), v)
        extra = 2.0 ** -20 * (1 + acc.abs())
        for got, want, slope, nm in ((gact, G.gelu_tanh(acc), dg.detach(), "gelu"), (u, dg.detach(), ddg, "gelu'")):
            err = (got.double().cpu() - want).abs()
            assert bool((err <= EPS_BF16 * want.abs() + t * d * slope.abs() + extra + 1e-30).all()), f"layer {l} {nm}"
    assert not any(isinstance(k, tuple) and k[0] == "ln1_mx" for k in ctx)  # every handed-over MX form was consumed


def _rel_grads(ga, gb):
    return {n: ((ga[n] - gb[n]).norm() / (gb[n].norm() + 1e-12)).item() for n in gb}


def test_loss_and_grads_vs_mx_fake_quant_oracle(cuda):
    """C3: loss and every parameter gradient against the MX fake-quant oracle, with the bound of
    tests/test_fp8_engine_gpu.py built the same way: 2e-2 + 3 e_n per parameter, e_n the same metric between two
    oracle runs on the CPU, MX fake-quant with fp32 quantiser inputs and with bf16-rounded ones.  Measured figures:
    docs/NUMERICS.md "MXFP8 forward"."""
    eng, mc = _engine(cuda, use_graph=False)
    b = next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999))
    eng.set_batch(b)
    st, T = eng.stage, mc.max_seq_len
    ctx = {}
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    h = st.stage_forward(h, 4, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (4 * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (4 * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    torch.cuda.synchronize()
    ids, lab = torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:])
    runs = []
    for bf in (False, True):
        params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
        lo = oracle_loss(mc, params, ids, lab, 0, 0, fake_quant="mx", quant_bf16_inputs=bf)
        lo.backward()
        runs.append((lo.item(), {n: params[n].grad for n in params}))
    (l32, g32), (l16, g16) = runs
    e_n = _rel_grads(g16, g32)
    e_loss = abs(l16 - l32)
    got = _rel_grads({n: eng.flat.g(n).cpu() for n in g32}, g32)
    print(f"MXFP8-C3 | loss gpu {loss.item():.6f} oracle {l32:.6f} bf16-input oracle {l16:.6f} | e_loss {e_loss:.3e}")
    for n in g32:
        print(f"MXFP8-C3 | {n} | gpu err {got[n]:.3e} | e_n {e_n[n]:.3e} | bound {2e-2 + 3 * e_n[n]:.3e}")
    assert abs(loss.item() - l32) <= 2e-2 + 3 * e_loss, (loss.item(), l32, e_loss)
    for n in g32:
        assert got[n] <= 2e-2 + 3 * e_n[n], f"{n}: relative grad error {got[n]:.3e}, e_n {e_n[n]:.3e}"


def test_graph_replay_determinism_and_launch_record(cuda):
    """C4: five steps under the graph equal five eager steps; two runs are bitwise identical; one forward runs the
    MX kernel 4 x layers times, fc1 with the fused MX output."""
    losses, params = {}, []
    for mode in (False, True, True):
        eng, mc = _engine(cuda, use_graph=mode)
        out = _steps(eng, mc, 5)
        if mode:
            assert eng.program.n_graphs >= 1
            params.append((out, eng.flat.params.clone()))
        losses[mode] = out
        del eng
    assert losses[True] == pytest.approx(losses[False], rel=1e-5, abs=1e-5), losses
    assert params[0][0] == params[1][0] and torch.equal(params[0][1], params[1][1])

    eng, mc = _engine(cuda, use_graph=False)
    eng.set_batch(next(get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)))
    calls = []
    real = MX._gemm_mxfp8
    try:
        MX._gemm_mxfp8 = lambda *a, **k: (real(*a, **k), calls.append(MX.last_launch_mxfp8()))[0]
        ctx = {}
        h = eng.stage.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
        eng.stage.stage_forward(h, 4, ctx)
    finally:
        MX._gemm_mxfp8 = real
    assert len(calls) == 4 * mc.n_layers
    assert [c.epilogue for c in calls] == ["bias", "bias", "gelu_pair", "bias"] * mc.n_layers
    assert all(c.variant == "mxfp8_64x128" for c in calls)
    assert [c.fused_quant for c in calls] == [False, False, True, False] * mc.n_layers


@pytest.mark.parametrize("add_ln", ["1", "0"], ids=["add_ln", "resid_epilogue"])
def test_fusion_changes_no_byte(cuda, monkeypatch, add_ln):
    """C4: five steps with DTC_MX_FUSE=0 (every activation through the stand-alone quantiser) give losses and final
    parameters bitwise equal to DTC_MX_FUSE=1, on the add-LayerNorm path and (DTC_ADD_LN=0) on the path where the
    GEMM epilogue adds the residual and a plain LayerNorm follows."""
    from distributed_training_compare_jax_amd.models import gpt

    monkeypatch.setattr(gpt, "_ADD_LN", add_ln == "1")
    runs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("DTC_MX_FUSE", fuse)
        eng, mc = _engine(cuda, use_graph=(add_ln == "1"))
        runs[fuse] = (_steps(eng, mc, 5), eng.flat.params.clone())
        del eng
    assert runs["1"][0] == runs["0"][0], runs
    assert torch.equal(runs["1"][1], runs["0"][1])


def test_thirty_steps_train(cuda):
    """C5: the loss falls by at least 0.5 in thirty steps; the bf16 and per-tensor-fp8 final losses are printed
    beside it, the gap is not asserted."""
    final = {}
    for fwd in ("mxfp8", "fp8", "bf16"):
        eng, mc = _engine(cuda, use_graph=True, fwd=fwd)
        vals = _steps(eng, mc, 30)
        final[fwd] = (vals[0], vals[-1])
        del eng
    print("MXFP8-C5 | " + " | ".join(f"{k} first {v[0]:.4f} last {v[1]:.4f}" for k, v in final.items()))
    assert final["mxfp8"][1] < final["mxfp8"][0] - 0.5, final


def test_wide_model_runs_through_the_layernorm_fallback(cuda):
    """C6: d_model 4096 (wider than the narrow LayerNorm kernels): one step with a finite loss, the LayerNorm outputs
    quantised by the stand-alone kernel."""
    eng, mc = _engine(cuda, use_graph=False, batch=1,
                      mc_kw=dict(d_model=4096, n_layers=1, n_heads=32, d_ff=4096, max_seq_len=64))
    assert mc.d_model // mc.n_heads == 128
    (loss,) = _steps(eng, mc, 1, batch=1)
    assert loss == loss and abs(loss) < 20.0, loss


def test_forward_ln_fusion_is_refused_by_name(cuda, monkeypatch):
    monkeypatch.setenv("DTC_LN_FUSE", "3")
    with pytest.raises(ValueError, match="DTC_LN_FUSE") as e:
        _engine(cuda)
    assert "fwd_gemm_dtype=mxfp8" in str(e.value)
