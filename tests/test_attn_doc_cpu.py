"""Document-masked attention without a GPU: the torch ``doc_bounds`` against a brute-force loop, the CPU
``attn_fwd`` / ``attn_bwd`` with ``doc`` against float64 autograd through a materialised masked softmax,
``TrainConfig.doc_mask_token`` and the engine's refusals, one CPU engine step against the masked autograd oracle, and
the plan functions of ``csrc/attn_plan.h`` in a plain C++ program (once more under ASan + UBSan)."""

import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.csrc import build as B
from distributed_training_compare_jax_amd.data import synthetic
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
SEP = 7
CPU = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")


def brute_bounds(ids, sep):
    rows, T = ids.shape
    ds, de = np.zeros((rows, T), np.int32), np.zeros((rows, T), np.int32)
    for b in range(rows):
        for t in range(T):
            s = t
            while s > 0 and ids[b, s - 1] != sep:
                s -= 1
            e = t + 1
            while e < T and ids[b, e - 1] != sep:
                e += 1
            ds[b, t], de[b, t] = s, e
    return ds, de


def _ids(rows, T, p, seed):
    g = np.random.default_rng(seed)
    ids = g.integers(SEP + 1, 60, (rows, T)).astype(np.int32)
    ids[g.random((rows, T)) < p] = SEP
    return ids


@pytest.mark.parametrize("T", [1, 2, 17, 64, 200])
def test_doc_bounds_against_a_brute_force_loop(T):
    ids = np.concatenate([_ids(3, T, p, T + i) for i, p in enumerate((0.0, 0.1, 0.6, 1.0))])
    ids[0, 0], ids[1, -1] = SEP, SEP  # a separator at position 0 and at T - 1
    ds, de = A.doc_bounds(torch.from_numpy(ids), SEP)
    want_s, want_e = brute_bounds(ids, SEP)
    assert ds.dtype == de.dtype == torch.int32
    assert np.array_equal(ds.numpy(), want_s) and np.array_equal(de.numpy(), want_e)
    pos = np.arange(T)
    assert (ds.numpy() <= pos).all() and (de.numpy() > pos).all()  # every query sees at least itself
    assert (np.diff(ds.numpy(), axis=1) >= 0).all() and (np.diff(de.numpy(), axis=1) >= 0).all()
    # the two forms of the definition: doc_start[q] <= k <= q  <=>  k <= q < doc_end[k]
    q, k = pos[:, None], pos[None, :]
    for b in range(ids.shape[0]):
        assert np.array_equal((want_s[b][:, None] <= k) & (k <= q), (k <= q) & (q < want_e[b][None, :]))


@pytest.mark.parametrize("hd", [16, 32, 64])
def test_cpu_attention_with_doc_against_float64_autograd(hd):
    Bn, T, H = 2, 70, 2
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(Bn, T, 3 * H * hd, generator=g)
    do = torch.randn(Bn, T, H * hd, generator=g)
    ids = _ids(Bn, T, 0.1, 5)
    doc = A.doc_bounds(torch.from_numpy(ids), SEP)
    o, lse = A.attn_fwd(qkv, H, doc=doc)
    dqkv = A.attn_bwd(qkv, o, lse, do, H, doc=doc)
    ds = torch.from_numpy(brute_bounds(ids, SEP)[0]).long()
    q, k, v = (t.clone().requires_grad_(True) for t in qkv.double().view(Bn, T, 3, H, hd).unbind(2))
    pos = torch.arange(T)
    see = (pos[None, None, :] >= ds[:, :, None]) & (pos[None, None, :] <= pos[None, :, None])
    s = (torch.einsum("bthd,bshd->bhts", q, k) * hd ** -0.5).masked_fill(~see[:, None], float("-inf"))
    o64 = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), v).reshape(Bn, T, H * hd)
    o64.backward(do.double())
    d64 = torch.stack([q.grad, k.grad, v.grad], 2).reshape(Bn, T, -1)
    # fp32 torch against float64: a few ulps of fp32 times the reduction lengths
    assert (o.double() - o64).abs().max() < 1e-5 and (lse.double() - torch.logsumexp(s, -1)).abs().max() < 1e-5
    assert (dqkv.double() - d64).abs().max() < 1e-4 * d64.abs().max()
    # doc=None is the plain causal call
    o0, _ = A.attn_fwd(qkv, H)
    assert not torch.equal(o0, o)
    one = (torch.zeros(Bn, T, dtype=torch.int32), torch.full((Bn, T), T, dtype=torch.int32))
    assert torch.equal(A.attn_fwd(qkv, H, doc=one)[0], o0)


def _cfgs(doc=SEP, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.0, **kw.pop("model", {}))
    tc = TrainConfig(seed=0, parallel=kw.pop("parallel", "dp"), batch=4, steps=1, log_every=1, output_dir="/tmp/unused",
                     device="cpu", warmup_steps=0, doc_mask_token=doc, **kw)
    return mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0)


def test_schema_default_and_values():
    assert TrainConfig(seed=0, parallel="dp", batch=4, steps=1, log_every=1, output_dir="/tmp/unused").doc_mask_token == -1
    for bad in (-2, True, 1.5, "7"):
        with pytest.raises(ValueError, match="doc_mask_token"):
            _cfgs(doc=bad)
    assert Engine(*_cfgs(doc=-1), CPU).doc_token == -1


def test_refusals_by_name():
    """Pipeline parallelism everywhere; dtype fp32 and a head_dim other than 64 / 128 on the GPU only (the engine
    reads the device's type and touches no device before it refuses).  The CPU engine takes the same layouts."""
    gpu = DistInfo(0, 1, 0, torch.device("cuda", 0), "nccl")
    mc, tc, oc = _cfgs(pp=2, parallel="pp")
    with pytest.raises(ValueError, match="doc_mask_token=7 cannot be combined with pp=2 .pipeline parallelism"):
        Engine(mc, tc, oc, DistInfo(0, 2, 0, torch.device("cpu"), "gloo"))
    mc, tc, oc = _cfgs(dtype="fp32", model=dict(d_model=128, n_heads=2))
    with pytest.raises(ValueError, match="doc_mask_token=7 cannot be combined with dtype=fp32 on the GPU"):
        Engine(mc, tc, oc, gpu)
    mc, tc, oc = _cfgs()  # tiny: head_dim 32
    assert mc.d_model // mc.n_heads == 32
    with pytest.raises(ValueError, match="doc_mask_token=7 cannot be combined with head_dim 32 on the GPU"):
        Engine(mc, tc, oc, gpu)
    Engine(mc, tc, oc, CPU)
    Engine(*_cfgs(dtype="fp32"), CPU)


def _batch(mc, rows=4, p=0.08, seed=3):
    return _ids(rows, mc.max_seq_len + 1, p, seed)


def _manual_step(eng, mc, b):
    eng.set_batch(b)
    st, T, n = eng.stage, mc.max_seq_len, b.shape[0]
    ctx = {}
    eng._doc_bounds_into(ctx, eng.ids)
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    h = st.stage_forward(h, n, ctx)
    loss = st.head_forward(h, eng.labels, 1 / (n * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (n * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    return float(loss)


def test_cpu_engine_step_matches_the_masked_oracle():
    """Loss and every gradient of one CPU step against autograd through the masked oracle, at the bounds of
    tests/test_model_cpu.py for the unmasked CPU engine (1e-5 on the loss, 1e-4 relative per gradient); the step
    program (run_step) gives the same loss; and the mask is not ignored: on parameters scaled up until attention
    matters, the unmasked oracle's loss is further away than that bound."""
    mc, tc, oc = _cfgs()
    eng = Engine(mc, tc, oc, CPU)
    for n in eng.flat.slots:  # the initial weights (std 0.02) give near-uniform attention: the mask would not show
        if n.endswith(".w") or n in ("wte", "wpe"):
            eng.flat.p(n).mul_(6.0)
    b = _batch(mc)
    assert (b[:, :-1] == SEP).mean() > 0.04
    loss = _manual_step(eng, mc, b)
    params = {n: eng.flat.p(n).detach().clone().requires_grad_(True) for n in eng.flat.slots}
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    lo = oracle_loss(mc, params, ids, lab, 0, 0, doc_mask_token=SEP)
    lo.backward()
    plain = float(oracle_loss(mc, {k: v.detach() for k, v in params.items()}, ids, lab, 0, 0))
    assert abs(loss - float(lo)) < 1e-5, (loss, float(lo))
    assert abs(loss - plain) > 1e-3, f"the masked loss {loss} is the unmasked oracle's {plain}: the mask is ignored"
    for n in eng.flat.slots:
        g, go = eng.flat.g(n), params[n].grad
        assert ((g - go).norm() / (go.norm() + 1e-12)).item() < 1e-4, n
    eng2 = Engine(mc, tc, oc, CPU)
    for n in eng2.flat.slots:
        eng2.flat.p(n).copy_(params[n].detach())
    eng2.set_batch(b)
    eng2.run_step()
    assert abs(eng2.loss_value() - float(lo)) < 1e-5
    # grad_accum: 2 microsteps compute their bounds from their own rows
    mc, tc, oc = _cfgs(grad_accum=2)
    eng3 = Engine(mc, tc, oc, CPU)
    for n in eng3.flat.slots:
        eng3.flat.p(n).copy_(params[n].detach())
    eng3.set_batch(b)
    eng3.run_step()
    assert abs(eng3.loss_value() - float(lo)) < 1e-5


# ------------------------------------------------------------------------------------------ gloo dp 2
DP_STEPS = 3


def _stream_sep():
    """The synthetic stream's most frequent token: an ordinary id that is frequent enough to cut every row."""
    return int(synthetic.SyntheticTokenStream(vocab=999, seed=0).rank_to_id[0])


def _dp_worker(doc, out_dir):
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed
    from distributed_training_compare_jax_amd.train.loop import train

    torch.set_num_threads(1)
    mc = model_config_from_preset("tiny", vocab_size=1000)
    tc = TrainConfig(seed=0, parallel="dp", batch=4, steps=DP_STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cpu", warmup_steps=0, doc_mask_token=doc)
    d = init_distributed("cpu")
    r = train(tc, mc, OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0), d, quiet=True, write_csv=False)
    eng = r["engine"]
    torch.save({"losses": r["history"], "params": {n: eng.flat.p(n).clone() for n in eng.flat.slots}},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    destroy()


def _dp_run(world, doc):
    with tempfile.TemporaryDirectory() as td:
        if world == 1:
            for k in ("WORLD_SIZE", "RANK"):
                os.environ.pop(k, None)
            _dp_worker(doc, td)
        else:
            spawn(_dp_worker, world, args=(doc, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(world)]


@pytest.mark.slow
def test_gloo_dp2_matches_dp1():
    """Three masked steps on two gloo ranks against one process, compared as
    tests/test_parallel_cpu.py::test_layout_matches_single_process compares the unmasked layouts: losses to 1e-4,
    parameters to rtol 1e-3 / atol 2e-5 (the ranks' fp32 gradient sums in another order).  Each rank computes the
    bounds from its own rows.  The same steps without the mask give other losses."""
    sep = _stream_sep()
    rows = synthetic.SyntheticTokenStream(vocab=999, seed=0).rows(0, 0, 4, 4, 65)
    assert (rows[:, :-1] == sep).sum() >= 4, "the separator is too rare in the first batch to show anything"
    one, two = _dp_run(1, sep)[0], _dp_run(2, sep)
    assert two[0]["losses"] == two[1]["losses"]
    assert two[0]["losses"] == pytest.approx(one["losses"], rel=1e-4, abs=1e-4)
    for n, a in one["params"].items():
        b = two[0]["params"][n]
        if n.endswith("qkv.b"):  # as that test: the key bias has an analytically-zero gradient, whose rounding noise
            a, b = a.view(3, -1)[[0, 2]], b.view(3, -1)[[0, 2]]  # Adam normalises to +-lr per step: q and v thirds only
        assert torch.allclose(b, a, rtol=1e-3, atol=2e-5), n
    plain = _dp_run(1, -1)[0]
    assert abs(plain["losses"][0] - one["losses"][0]) > 1e-4, "the mask changed nothing"


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")


def _plan_check(tmp_path, *flags):
    exe = str(tmp_path / "attn_doc_plan_check")
    src = os.path.join(HERE, "native", "attn_doc_plan_check.cpp")
    if flags:  # is the sanitizer runtime there at all?  A trivial program says; the real one is then never skipped
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        pr = subprocess.run([_cxx(), *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode != 0:
            pytest.skip(f"sanitizer runtime unavailable: {pr.stderr[-300:]}")
    r = subprocess.run([_cxx(), "-O1", "-g", "-std=c++17", *flags, "-I", B.HERE, src, "-o", exe], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok"), run.stdout[-1000:]


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_doc_plans(tmp_path):
    """tests/native/attn_doc_plan_check.cpp: the doc plans name the expected kernels, grids and blocks over a sweep of
    (B, T, H, HD, flags, knobs, CUs), other head_dims are refused with 4005, and the unmasked plans name no doc
    path or kernel (tests/test_attn_plan_cpu.py holds them to the parent's listing)."""
    _plan_check(tmp_path)


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_doc_plans_asan_ubsan(tmp_path):
    """The same program under AddressSanitizer + UndefinedBehaviorSanitizer, as its own process."""
    _plan_check(tmp_path, "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_python_tables_name_the_doc_kernels():
    assert A.PATHS[-3:] == ("fwd_rows32_doc", "bwd_rows32_doc_128", "bwd_rows32_doc_merged")
    assert A.KERNELS[-5:] == ("attn_fwd32_doc_kernel<64>", "attn_fwd32_doc_kernel<128>", "attn_bwd_dq32_doc_kernel<128>",
                              "attn_bwd_dkdv32_doc_kernel<128>", "attn_bwd_merged32_doc_kernel<64>")
