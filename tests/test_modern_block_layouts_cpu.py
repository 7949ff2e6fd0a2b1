"""The modern block (``pos_emb: rope``, ``norm: rmsnorm``, ``mlp: swiglu``, ``qk_norm: rmsnorm``) through the real
``Engine.run_step`` without a GPU: the accumulated step against the float64 autograd oracle, and the pipeline schedules
against the single-process run.  The ``beta`` that the second and later microbatches hand to the gain, norm and
weight-gradient outputs is Python plumbing shared by both devices, so a wrong one fails here first.  (The GPU twin,
tests/test_modern_block_layouts_gpu.py, imports the models below.)

``wgrad_group=-1`` cases: by default the weight gradients are deferred to a grouped launch that takes ``beta`` as an
argument; with the deferral off ``GPTStage._wg`` launches each one with ``self._beta``, which is then the only carrier
of the microbatch's ``beta`` for the SwiGLU ``fc2`` weight gradient."""

import pytest
import torch
from test_parallel_cpu import _full_params, _run
from test_qknorm_cpu import _move_gains

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine

# the smallest shapes the kernels take that still have a Q/K-boundary-straddling QK-norm pass, a fused SwiGLU pair
# (F % 64, D % 64) and the GQA 32-row attention family
MODERN = dict(pos_emb="rope", norm="rmsnorm", mlp="swiglu", qk_norm="rmsnorm")
SHAPE = dict(max_seq_len=128, d_model=256, d_ff=512)
FULL_BF16 = dict(SHAPE, n_heads=4, n_kv_heads=2, **MODERN)  # head_dim 64, GQA
FULL_HD128 = dict(SHAPE, n_heads=2, n_kv_heads=1, **MODERN)  # head_dim 128, GQA
FULL_F32 = dict(SHAPE, n_heads=4, **MODERN)  # MHA: the GPU refuses GQA under dtype=fp32
FULL_CPU = dict(FULL_F32, n_kv_heads=2)  # the CPU path takes GQA in fp32
WATCHED = ("qn.g", "kn.g", "ln1.g", "ln2.g", "lnf.g", "fc1.w", "fc2.w", "out.b", "fc2.b")  # printed by name

LOSS_TOL, GRAD_TOL = 1e-5, 1e-4  # tests/test_qknorm_cpu.py test_cpu_gradients_match_the_oracle


def model(over, layers=2):
    return model_config_from_preset("tiny", vocab_size=1000, n_layers=layers, **over)  # dropout 0.1


def oracle(mc, p0, b, **kw):
    """float64 loss and gradients of the whole batch (dropout mask of step 0, row 0)."""
    params = {n: t.double().requires_grad_(True) for n, t in p0.items()}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous(), 0, 0,
                     **kw)
    lo.backward()
    return lo.item(), {n: params[n].grad for n in params}


def grad_errors(grads, ref_grads):
    """Relative L2 error per parameter.  ``qkv.b`` in full: the rotation and the head norm both break the softmax's
    shift invariance, so the key bias's gradient is not zero here."""
    return {n: ((grads[n].double() - go).norm() / (go.norm() + 1e-300)).item() for n, go in ref_grads.items()}


def one_step(mc, device, k, batch=8, b=None, **kw):
    """One real ``run_step`` at ``grad_accum=k`` from moved gains, on the stream's first batch or on ``b`` ->
    (engine, batch, initial parameters, loss, gradients)."""
    dev = torch.device(device)
    tc = TrainConfig(**{**dict(seed=0, parallel="dp", batch=batch, steps=1, log_every=1, output_dir="/tmp/x",
                               device=dev.type, use_graph=False, grad_accum=k), **kw})
    eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0),
                 DistInfo(0, 1, 0, dev, "gloo" if dev.type == "cpu" else "nccl"))
    _move_gains(eng, mc)  # away from their init of ones, so that they are seen to act
    eng.flat.refresh_mirror()
    b = next(get_batch_iterator(batch, mc.max_seq_len + 1, vocab=999)) if b is None else b
    p0 = {n: eng.flat.p(n).detach().float().cpu().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    loss = eng.loss_value()
    assert (eng.n_micro, eng.mb_rows) == (k, batch // k) and int(eng.opt.step_t.item()) == 1
    return eng, b, p0, loss, {n: eng.flat.g(n).detach().float().cpu().clone() for n in eng.flat.slots}


def print_watched(what, errs, base=None):
    for n in errs:
        if n.endswith(WATCHED):
            print(f"MODERN | {what} | {n} | error {errs[n]:.3e}"
                  + ("" if base is None else f" | k=1 error {base[n]:.3e} | ratio {errs[n] / base[n]:.3f}"))


@pytest.mark.parametrize("batch,k,kw", [(8, 2, {}), (8, 4, {}), (8, 2, dict(wgrad_group=-1))],
                         ids=["k2", "k4", "k2_wgrad_now"])
def test_accumulated_step_matches_oracle(batch, k, kw):
    mc = model(FULL_CPU)
    eng, b, p0, loss, grads = one_step(mc, "cpu", k, batch, dtype="fp32", **kw)
    assert eng.stage._defer_wg == (not kw) and "h.0.qn.g" in grads and "wpe" not in grads and "h.0.ln1.b" not in grads
    ref_loss, ref_grads = oracle(mc, p0, b)
    errs = grad_errors(grads, ref_grads)
    print_watched(f"cpu fp32 batch {batch} k {k} {kw}", errs)
    assert abs(loss - ref_loss) < LOSS_TOL, (loss, ref_loss)
    for n, e in errs.items():
        assert e < GRAD_TOL, f"k {k} {n}: relative grad error {e:.3e}"


@pytest.fixture(scope="module")
def single():
    return _run("dp", 1, model=FULL_CPU, eps=1e-4)


@pytest.mark.slow
@pytest.mark.parametrize("kw", [{"pp_schedule": "1f1b"}, {"pp_schedule": "zb"}, {"pp_schedule": "1f1b", "wgrad_group": -1}],
                         ids=["1f1b", "zb", "1f1b_wgrad_now"])
def test_pp2_matches_single_process(single, kw):
    """Four microbatches on two stages, two layers each, with tests/test_parallel_cpu.py's harness and the tolerances
    it holds the GQA + rope + rmsnorm + swiglu block to (``test_uneven_heads_match_single_process``: Adam eps 1e-4
    keeps the update linear in near-zero gradients, so the parameters compare at fp32 rounding level; at eps 1e-8
    one element of ``h.1.qkv.w`` and three of ``wte`` moved by up to 1.2e-4 between the two runs).  ``qkv.b`` is
    compared in full."""
    res = _run("pp", 2, model=FULL_CPU, eps=1e-4, pp_microbatches=4, pp_clip="global", **kw)
    assert [r["mesh"] for r in res] == [(1, 1, 2)] * 2
    assert res[0]["losses"] == pytest.approx(single[0]["losses"], rel=1e-5, abs=1e-5)
    full, ref = _full_params(res, model=FULL_CPU), single[0]["params"]
    assert set(full) == set(ref) and "h.3.kn.g" in ref and "wpe" not in ref
    for n in ref:
        assert torch.allclose(full[n], ref[n], rtol=1e-5, atol=1e-6), (n, (full[n] - ref[n]).abs().max().item())
