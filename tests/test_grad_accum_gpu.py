"""``grad_accum: k`` on the HIP path: the accumulated step against the float64 oracle (held to 2x the error of the
unaccumulated step of the same precision, measured in the same test: the runs differ in summation order only),
one hipGraph, the activation memory, the multi-process layouts on one GPU, MXFP8 and the debug library."""

import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributed_training_compare_jax_amd")


def _mc(layers=2):
    return model_config_from_preset("tiny", vocab_size=1000, n_layers=layers)  # dropout 0.1


def _engine(dev, k, batch=8, use_graph=False, layers=2, **kw):
    mc = _mc(layers)
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=1, log_every=1, output_dir="/tmp/x",
                     use_graph=use_graph, grad_accum=k, **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


def _batch(mc, batch):
    return next(get_batch_iterator(batch, mc.max_seq_len + 1, vocab=999))


def _one_step(dev, k, batch=8, **kw):
    eng, mc = _engine(dev, k, batch, **kw)
    b = _batch(mc, batch)
    p0 = {n: eng.flat.p(n).detach().float().cpu().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    loss = eng.loss_value()
    torch.cuda.synchronize()
    assert (eng.n_micro, eng.mb_rows) == (k, batch // k) and int(eng.opt.step_t.item()) == 1
    return mc, b, p0, loss, {n: eng.flat.g(n).detach().float().cpu().clone() for n in eng.flat.slots}


def _oracle(mc, p0, b, **kw):
    # float64, except under the fake-quant oracle, whose quantiser is written for fp32 tensors
    params = {n: (t.float() if kw.get("fake_quant") else t.double()).requires_grad_(True) for n, t in p0.items()}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0, **kw)
    lo.backward()
    return lo.item(), {n: params[n].grad for n in params}


def _errors(grads, loss, ref_loss, ref_grads):
    out = {}
    for n, go in ref_grads.items():
        g = grads[n].double()
        if n.endswith("qkv.b"):  # the key bias's gradient is analytically zero (softmax shift invariance)
            g, go = g.view(3, -1)[[0, 2]], go.view(3, -1)[[0, 2]]
        out[n] = ((g - go).norm() / (go.norm() + 1e-300)).item()
    return out, abs(loss - ref_loss)


@functools.lru_cache(maxsize=None)
def _base(dtype, batch):
    """The k = 1 step of this precision and batch, its oracle and its errors (computed once, never modified)."""
    dev = torch.device("cuda", 0)
    mc, b, p0, loss, grads = _one_step(dev, 1, batch, dtype=dtype)
    ref_loss, ref_grads = _oracle(mc, p0, b)
    errs, lerr = _errors(grads, loss, ref_loss, ref_grads)
    return dict(mc=mc, ref_loss=ref_loss, ref_grads=ref_grads, errs=errs, lerr=lerr, loss=loss)


def _check_ratio(base, grads, loss, what):
    errs, lerr = _errors(grads, loss, base["ref_loss"], base["ref_grads"])
    ratios = {n: errs[n] / base["errs"][n] for n in errs}
    worst = max(ratios, key=ratios.get)
    print(f"ACCUM-RATIO | {what} | grad error / k=1 error in [{min(ratios.values()):.3f}, {ratios[worst]:.3f}] "
          f"(worst {worst}: {errs[worst]:.3e} vs {base['errs'][worst]:.3e}) | loss error {lerr:.3e} vs "
          f"{base['lerr']:.3e}")
    for n in errs:
        assert errs[n] <= 2.0 * base["errs"][n], f"{what} {n}: {errs[n]:.3e} > 2 x {base['errs'][n]:.3e}"
    # the fp32 loss scalar has a rounding of its own (2^-24 relative) below which no error can be held
    assert lerr <= 2.0 * max(base["lerr"], abs(base["ref_loss"]) * 2.0 ** -24), (lerr, base["lerr"])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("batch,k", [(8, 2), (8, 4), (4, 4)], ids=["M256", "M128", "M64"])
def test_accumulated_step_matches_oracle(cuda, dtype, batch, k):
    base = _base(dtype, batch)
    mc, b, p0, loss, grads = _one_step(cuda, k, batch, dtype=dtype)
    _check_ratio(base, grads, loss, f"{dtype} batch {batch} k {k}")


def test_mxfp8_accumulated_step_matches_its_oracle(cuda):
    """d_model 128 / d_ff 512 are the smallest the FP8 GEMM's k-step takes; the oracle is the MX fake-quant one."""
    mk = dict(d_model=128, d_ff=512, n_heads=4)
    out = {}
    for k in (1, 2):
        mc = model_config_from_preset("tiny", vocab_size=1000, **mk)
        tc = TrainConfig(seed=0, parallel="dp", batch=8, steps=1, log_every=1, output_dir="/tmp/x", use_graph=False,
                         grad_accum=k, fwd_gemm_dtype="mxfp8")
        eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, cuda, "nccl"))
        b = _batch(mc, 8)
        p0 = {n: eng.flat.p(n).detach().float().cpu().clone() for n in eng.flat.slots}
        eng.set_batch(b)
        eng.run_step()
        out[k] = (eng.loss_value(), {n: eng.flat.g(n).detach().float().cpu().clone() for n in eng.flat.slots})
    ref_loss, ref_grads = _oracle(mc, p0, b, fake_quant="mx", quant_bf16_inputs=True)
    errs, lerr = _errors(out[1][1], out[1][0], ref_loss, ref_grads)
    _check_ratio(dict(ref_loss=ref_loss, ref_grads=ref_grads, errs=errs, lerr=lerr), out[2][1], out[2][0], "mxfp8 k 2")


def test_graph_replay_matches_eager_in_one_graph(cuda):
    losses = {}
    for mode in (False, True):
        eng, mc = _engine(cuda, 2, batch=4, use_graph=mode)
        it = get_batch_iterator(4, mc.max_seq_len + 1, vocab=999)
        out = []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        losses[mode] = out
        if mode:
            assert eng.program.n_graphs == 1 and eng.program.n_comms == 0, (eng.program.n_graphs, eng.program.n_comms)
            assert int(eng.opt.step_t.item()) == 5
    assert losses[True] == pytest.approx(losses[False], rel=1e-5, abs=1e-5), losses


def test_fused_embedding_paths_see_one_backward(cuda, monkeypatch):
    """dp 1: the embedding backward keeps its fused Σg² partials and sparse zeroing, because it still runs once per
    step over the whole local batch with beta = 0 (never with beta = 1)."""
    from distributed_training_compare_jax_amd.ops import embedding as E

    eng, mc = _engine(cuda, 4, batch=8, use_graph=False)
    calls, real = [], E.embed_bwd

    def spy(ids, dh, gwte, gwpe, p, seed, step, row0, beta, **kw):
        calls.append((tuple(dh.shape), beta, kw.get("sq") is not None, kw.get("prev_keys") is not None))
        return real(ids, dh, gwte, gwpe, p, seed, step, row0, beta, **kw)

    monkeypatch.setattr(E, "embed_bwd", spy)
    it = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999)
    for _ in range(3):
        eng.set_batch(next(it))
        eng.run_step()
    eng.loss_value()
    assert len(calls) == 3 and all(c[0] == (8 * eng.T, mc.d_model) and c[1] == 0.0 for c in calls), calls
    assert calls[-1][3], "sparse wte zeroing is off"
    if eng.stage.wg_record:
        assert calls[-1][2], "the fused embedding grad-norm partials are off"


MEM_BATCH = 1280


def test_activation_memory_scales_with_the_microbatch(cuda):
    """Eager, k = 4 against k = 1.  ``static`` = bytes allocated after construction; the transient part of k = 1
    must be at least as large as it (else the comparison means nothing), and k = 4 may use at most half of that
    transient: activations scale as 1/k, the other quarter is what stays full-batch (ids, labels, the
    embedding-gradient buffer).  Batch 1280: the engine holds about 0.6 GB for good (the 512 MiB batched-reduction
    arena and, in a fresh process, the 96 MiB GEMM workspace), and the tiny preset's activations are 0.63 MB per
    sequence (measured: 480 MB at batch 768), so this is the batch at which the transient part outweighs it."""
    res = {}
    for k in (1, 4):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        eng, mc = _engine(cuda, k, batch=MEM_BATCH, use_graph=False)
        torch.cuda.synchronize()
        static = torch.cuda.memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        eng.set_batch(_batch(mc, MEM_BATCH))
        eng.run_step()
        eng.loss_value()
        torch.cuda.synchronize()
        res[k] = (static, torch.cuda.max_memory_allocated() - start)
        del eng
    print(f"ACCUM-MEM | static k1 {res[1][0]} k4 {res[4][0]} | transient k1 {res[1][1]} k4 {res[4][1]} | "
          f"ratio {res[4][1] / res[1][1]:.3f}")
    assert res[1][1] >= res[1][0], f"transient {res[1][1]} < static {res[1][0]}: the measurement means nothing"
    assert res[4][1] <= 0.5 * res[1][1], res


# ------------------------------------------------------------------------------------ processes on one GPU
def _worker(kw, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    kw = dict(kw)
    parallel = kw.pop("parallel", "dp")
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed

    mc = _mc(4)
    tc = TrainConfig(seed=0, parallel=parallel, batch=8, steps=6, log_every=1000, output_dir="/tmp/unused",
                     device="cuda", warmup_steps=0, dp_bucket_mb=0.25, dp_tail_mb=0.05, **kw)
    d = init_distributed("cuda")
    eng = Engine(mc, tc, OptimConfig(lr=3e-3, weight_decay=0.1, grad_clip=1.0), d)
    it = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999)
    losses, first, b0 = [], None, None
    for s in range(6):
        b = next(it)
        b0 = b if b0 is None else b0
        eng.set_batch(b[eng.feed_row0:eng.feed_row0 + eng.feed_rows])
        eng.run_step()
        losses.append(eng.loss_value())
        if s == 0:
            first = {n: eng.flat.g(n).detach().float().cpu().clone() for n in eng.flat.slots}
            if eng.zero:  # a rank's buffer holds the reduced gradient on the slices it owns: keep those apart
                flat = eng.flat.grads.detach().cpu().clone()
                first = {"flat": flat, "owned": [tuple(o) for o in eng.opt.owned],
                         "slots": {n: (sl.offset, sl.numel, tuple(eng.flat.g(n).shape))
                                   for n, sl in eng.flat.slots.items()}}
    eng.check_health()
    torch.save({"losses": losses, "graphs": eng.program.n_graphs, "comms": eng.program.n_comms, "grads": first,
                "params": eng.flat.params.cpu(), "tp_idx": eng.mesh.tp_idx, "dp_idx": eng.mesh.dp_idx,
                "sp": eng.stage.sp, "n_micro": eng.n_micro, "zero": eng.zero, "b0": b0},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


def _spawn2(kw):
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, 2, args=(kw, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(2)]


def _full_grads(results, mc):
    from distributed_training_compare_jax_amd.models.params import all_param_specs, unshard

    specs = {s.name: s for s in all_param_specs(mc)}
    pieces = {}
    for r in results:
        if r["dp_idx"] == 0:
            for n, t in r["grads"].items():
                pieces.setdefault(n, {})[r["tp_idx"]] = t
    return {n: unshard(specs[n], [p[i] for i in sorted(p)]) for n, p in pieces.items()}


@functools.lru_cache(maxsize=None)
def _base4():
    """k = 1, one process, 4 layers, bf16, batch 8: the reference error of the multi-process cases."""
    dev = torch.device("cuda", 0)
    mc, b, p0, loss, grads = _one_step(dev, 1, 8, layers=4)
    ref_loss, ref_grads = _oracle(mc, p0, b)
    errs, lerr = _errors(grads, loss, ref_loss, ref_grads)
    return dict(mc=mc, ref_loss=ref_loss, ref_grads=ref_grads, errs=errs, lerr=lerr)


@pytest.mark.slow
@pytest.mark.parametrize("kw", [dict(dp_comm="p2p"), dict(zero_stage=1, zero_comm="p2p")], ids=["dp_p2p", "zero_p2p"])
def test_dp2_p2p_accumulated_in_one_graph(cuda, kw):
    res = _spawn2(dict(kw, grad_accum=2))
    for r in res:
        assert r["n_micro"] == 2 and r["graphs"] == 1 and r["comms"] == 0, (r["graphs"], r["comms"])
    assert torch.equal(res[0]["params"], res[1]["params"]) and res[0]["losses"] == res[1]["losses"]
    grads = res[0]["grads"]
    if "zero_stage" in kw:  # the reduced gradient, assembled from the slices each rank owns
        flat = torch.full_like(grads["flat"], float("nan"))
        for r in res:
            for lo, hi in r["grads"]["owned"]:
                flat[lo:hi] = r["grads"]["flat"][lo:hi]
        grads = {n: flat[o:o + k].view(shape) for n, (o, k, shape) in grads["slots"].items()}
    _check_ratio(_base4(), grads, res[0]["losses"][0], f"dp2 {kw} k 2")


@pytest.mark.slow
def test_tp2_sequence_parallel_accumulated(cuda):
    res = _spawn2(dict(parallel="tp", tp_sequence_parallel=True, grad_accum=2))
    assert all(r["sp"] and r["n_micro"] == 2 for r in res)
    assert res[0]["losses"] == res[1]["losses"]
    _check_ratio(_base4(), _full_grads(res, _base4()["mc"]), res[0]["losses"][0], "tp2 sp k 2")


# ------------------------------------------------------------------------------------------ debug library
SCRIPT = r"""
import torch
from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.parallel.dist import DistInfo
from distributed_training_compare_jax_amd.train.engine import Engine
from distributed_training_compare_jax_amd.ops import _native as N

dev = torch.device("cuda:0")
mc = model_config_from_preset("tiny", vocab_size=1000)
tc = TrainConfig(seed=0, parallel="dp", batch=8, steps=3, log_every=1, output_dir="/tmp/x", use_graph=True, grad_accum=4)
oc = OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0, lr_schedule="warmup_cosine", lr_warmup_steps=1,
                 lr_decay_steps=3)
eng = Engine(mc, tc, oc, DistInfo(0, 1, 0, dev, "nccl"))
it = get_batch_iterator(8, mc.max_seq_len + 1, vocab=999)
losses = []
for _ in range(3):
    eng.set_batch(next(it))
    eng.run_step()
    losses.append(eng.loss_value())
torch.cuda.synchronize()
print("LIB", N.LIB_PATH)
print("LOSSES", " ".join(f"{x:.6f}" for x in losses))
"""


def _run_lib(lib):
    env = dict(os.environ, DTC_KERNEL_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{os.path.basename(lib)} exited {r.returncode}:\n{out[-4000:]}"
    libs = [l for l in r.stdout.splitlines() if l.startswith("LIB ")]
    assert libs and libs[0].split()[1] == lib, out[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("LOSSES ")]
    assert line, out[-4000:]
    return [float(x) for x in line[0].split()[1:]]


def test_debug_library_runs_accumulated_steps_clean(cuda):
    """The -DDTC_DEBUG library (every DTC_ASSERT live) through accumulated, scheduled, graph-replayed steps: a
    one-sequence microbatch's index math (M = 128 here) stays inside its buffers; losses match the release build."""
    dbg, rel = os.path.join(PKG, "_dtc_kernels_debug.so"), os.path.join(PKG, "_dtc_kernels.so")
    assert os.path.exists(dbg), "debug kernel library missing: __graft_entry__.build() builds it in-tree"
    ld, lr = _run_lib(dbg), _run_lib(rel)
    for a, b in zip(ld, lr):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (ld, lr)
