"""``grad_accum: k`` on the CPU engine: the accumulated step against the float64 autograd oracle, the refusals,
and what the default leaves untouched.

The k microbatches of a step differ from the unaccumulated step only in the order of fp32 sums (the dropout mask is
the same: every microstep passes the global row offset of its first row), so their rounding noise against the
float64 oracle (``models/reference.py`` on double parameters) is of the same size: each parameter's relative L2
gradient error at k > 1 is held to 2x the k = 1 error measured in the same test, and the loss error likewise."""

import os
import tempfile

import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

BATCH = 8


def _cfgs(k=1, batch=BATCH, parallel="dp", layers=2, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, n_layers=layers)  # dropout 0.1
    tc = TrainConfig(seed=0, parallel=parallel, batch=batch, steps=1, log_every=1000, output_dir="/tmp/unused",
                     device="cpu", warmup_steps=0, dtype="fp32", grad_accum=k, **kw)
    oc = OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0)
    return mc, tc, oc


def _batch(mc, batch=BATCH):
    return next(get_batch_iterator(batch, mc.max_seq_len + 1, vocab=999))


def _engine(k=1, **kw):
    mc, tc, oc = _cfgs(k, **kw)
    return Engine(mc, tc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo")), mc


def _oracle(mc, p0, b):
    """float64 loss and gradients of the whole batch (dropout mask of step 0, row 0)."""
    params = {n: t.double().requires_grad_(True) for n, t in p0.items()}
    lo = oracle_loss(mc, params, torch.from_numpy(b[:, :-1]), torch.from_numpy(b[:, 1:]), 0, 0)
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


def _one_step(k, **kw):
    eng, mc = _engine(k, **kw)
    b = _batch(mc, eng.global_batch)
    p0 = {n: eng.flat.p(n).detach().clone() for n in eng.flat.slots}
    eng.set_batch(b)
    eng.run_step()
    loss = eng.loss_value()
    return eng, mc, b, p0, loss, {n: eng.flat.g(n).detach().clone() for n in eng.flat.slots}


@pytest.fixture(scope="module")
def base():
    """The k = 1 step, its float64 oracle and its errors (shared, never modified)."""
    eng, mc, b, p0, loss, grads = _one_step(1)
    ref_loss, ref_grads = _oracle(mc, p0, b)
    errs, lerr = _errors(grads, loss, ref_loss, ref_grads)
    return dict(mc=mc, b=b, p0=p0, ref_loss=ref_loss, ref_grads=ref_grads, errs=errs, lerr=lerr)


def _check_ratio(base, grads, loss, what):
    errs, lerr = _errors(grads, loss, base["ref_loss"], base["ref_grads"])
    ratios = {n: errs[n] / base["errs"][n] for n in errs}
    worst = max(ratios, key=ratios.get)
    print(f"{what}: grad error ratio to k=1 in [{min(ratios.values()):.3f}, {ratios[worst]:.3f}] (worst {worst}: "
          f"{errs[worst]:.3e} vs {base['errs'][worst]:.3e}); loss error {lerr:.3e} vs {base['lerr']:.3e}")
    for n in errs:
        assert errs[n] <= 2.0 * base["errs"][n], f"{what} {n}: {errs[n]:.3e} > 2 x {base['errs'][n]:.3e}"
    # the fp32 loss has one rounding of its own (2^-24 relative) below which an error cannot be held
    assert lerr <= 2.0 * max(base["lerr"], abs(base["ref_loss"]) * 2.0 ** -24), (lerr, base["lerr"])


@pytest.mark.parametrize("k", [2, 4, 8])
def test_accumulated_step_matches_oracle(base, k):
    eng, mc, b, p0, loss, grads = _one_step(k)
    assert (eng.n_micro, eng.mb_rows) == (k, BATCH // k)
    assert int(eng.opt.step_t.item()) == 1
    _check_ratio(base, grads, loss, f"k={k}")


def test_step_counter_counts_updates():
    eng, mc = _engine(4)
    it = get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
    for n in range(1, 4):
        eng.set_batch(next(it))
        eng.run_step()
        assert int(eng.opt.step_t.item()) == n


def test_six_steps_bitwise_reproducible():
    runs = []
    for _ in range(2):
        eng, mc = _engine(2)
        it = get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
        losses = []
        for _ in range(6):
            eng.set_batch(next(it))
            eng.run_step()
            losses.append(eng.loss_value())
        runs.append((losses, eng.flat.params.clone(), eng.flat.exp_avg_sq.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_training_follows_unaccumulated_run():
    """Six updates at k = 4 track the k = 1 run of the same data (same masks, same update count)."""
    out = {}
    for k in (1, 4):
        eng, mc = _engine(k)
        it = get_batch_iterator(BATCH, mc.max_seq_len + 1, vocab=999)
        losses = []
        for _ in range(6):
            eng.set_batch(next(it))
            eng.run_step()
            losses.append(eng.loss_value())
        out[k] = losses
    assert out[4] == pytest.approx(out[1], rel=1e-4, abs=1e-4)


# ---------------------------------------------------------------- multi-process (gloo)
def _worker(parallel, kw, out_dir):
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed

    torch.set_num_threads(1)
    mc, tc, oc = _cfgs(parallel=parallel, **kw)
    d = init_distributed("cpu")
    eng = Engine(mc, tc, oc, d)
    b = _batch(mc)
    eng.set_batch(b[eng.feed_row0:eng.feed_row0 + eng.feed_rows])
    eng.run_step()
    loss = eng.loss_value()
    torch.save({"loss": loss, "grads": {n: eng.flat.g(n).clone() for n in eng.flat.slots}, "tp_idx": eng.mesh.tp_idx,
                "dp_idx": eng.mesh.dp_idx, "sp": eng.stage.sp, "n_micro": eng.n_micro},
               os.path.join(out_dir, f"rank{d.rank}.pt"))
    destroy()


def _full_grads(results, mc):
    from distributed_training_compare_jax_amd.models.params import all_param_specs, unshard

    specs = {s.name: s for s in all_param_specs(mc)}
    pieces = {}
    for r in results:
        if r["dp_idx"] == 0:
            for n, t in r["grads"].items():
                pieces.setdefault(n, {})[r["tp_idx"]] = t
    return {n: unshard(specs[n], [p[i] for i in sorted(p)]) for n, p in pieces.items()}


@pytest.mark.parametrize("parallel,kw", [("dp", {}), ("tp", {"tp_sequence_parallel": True})])
def test_two_ranks_accumulated_step_matches_oracle(base, parallel, kw):
    with tempfile.TemporaryDirectory() as td:
        spawn(_worker, 2, args=(parallel, dict(kw, k=2), td))
        res = [torch.load(os.path.join(td, f"rank{r}.pt"), weights_only=False) for r in range(2)]
    assert all(r["n_micro"] == 2 for r in res)
    if parallel == "tp":
        assert all(r["sp"] for r in res)
    _check_ratio(base, _full_grads(res, base["mc"]), res[0]["loss"], f"{parallel}2 k=2")


# ---------------------------------------------------------------- refusals and defaults
class _NoCollectives:
    """Any process-group call while this is active fails the test: the refusals come before all of them."""

    def __enter__(self):
        import torch.distributed as dist

        self.saved = {n: getattr(dist, n) for n in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast",
                                                    "barrier", "new_group", "reduce_scatter_tensor")}

        def boom(*a, **k):
            raise AssertionError("a collective ran before the refusal")

        for n in self.saved:
            setattr(dist, n, boom)

    def __exit__(self, *a):
        import torch.distributed as dist

        for n, f in self.saved.items():
            setattr(dist, n, f)


@pytest.mark.parametrize("kw,match", [
    (dict(k=3), "grad_accum=3.*whole microbatches"),
    (dict(k=0), "grad_accum=0.*>= 1"),
    (dict(k=-2), "grad_accum=-2"),
    (dict(k=2, parallel="pp", pp=1, defer_optimizer=True), "defer_optimizer"),
])
def test_refusals(kw, match):
    with _NoCollectives(), pytest.raises(ValueError, match=match):
        _engine(**kw)


def test_refuses_pipeline_parallel_by_name():
    mc, tc, oc = _cfgs(2, parallel="pp", pp=2, pp_microbatches=2)
    with _NoCollectives(), pytest.raises(ValueError, match="pp_microbatches"):
        Engine(mc, tc, oc, DistInfo(0, 2, 0, torch.device("cpu"), "gloo"))


def test_defaults_are_untouched():
    assert TrainConfig(seed=0, parallel="dp", batch=8, steps=1, log_every=1, output_dir="x").grad_accum == 1
    eng, _ = _engine(1)
    assert (eng.grad_accum, eng.n_micro, eng.mb_rows) == (1, 1, BATCH)
    assert not hasattr(eng, "dh_acc")  # no full-batch embedding-gradient buffer without accumulation
    eng4, _ = _engine(4)
    assert eng4.dh_acc.shape == (BATCH * eng4.T, eng4.mcfg.d_model)
    assert eng4.flat.numel == eng.flat.numel and eng4.ids.shape == eng.ids.shape


def test_embedding_backward_runs_once_with_beta_zero(monkeypatch):
    """The fused Σg² / sparse-zeroing paths of the embedding backward need ONE writer per step: under accumulation the
    engine still calls it once, over the whole local batch, with beta = 0."""
    from distributed_training_compare_jax_amd.ops import embedding as E

    eng, mc = _engine(4)
    calls = []
    real = E.embed_bwd

    def spy(ids, dh, gwte, gwpe, p, seed, step, row0, beta, **kw):
        calls.append((tuple(ids.shape), tuple(dh.shape), row0, beta))
        return real(ids, dh, gwte, gwpe, p, seed, step, row0, beta, **kw)

    monkeypatch.setattr(E, "embed_bwd", spy)
    eng.set_batch(_batch(mc))
    eng.run_step()
    assert calls == [((BATCH, eng.T), (BATCH * eng.T, mc.d_model), 0, 0.0)], calls


def test_metrics_record_accumulation(tmp_path):
    import json

    from distributed_training_compare_jax_amd.train.loop import train

    mc, tc, oc = _cfgs(2)
    from dataclasses import replace

    tc = replace(tc, steps=2, output_dir=str(tmp_path))
    train(tc, mc, oc, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"), quiet=True)
    m = json.load(open(tmp_path / "metrics.json"))
    assert (m["grad_accum"], m["microbatch_rows"]) == (2, 4)
    assert open(tmp_path / "log.csv").readline().strip() == "step,elapsed_time,loss"
