"""``TrainConfig.doc_mask_token`` end to end on the GPU: two small models (2 heads of 64 and 2 heads of 128, two
layers, T 200: two 128-query attention blocks, the second ragged) against the masked autograd oracle at the
tolerances tests/test_engine_gpu.py uses for the unmasked model, hipGraph replay against eager, run-to-run bits,
grad_accum 2 against 1, Engine.evaluate against the training forward, ``doc_mask_token: -1`` against a config
without the field, and tp 2 over P2P (with and without sequence parallelism, two processes on one device, the rig of
tests/test_eval_dist_gpu.py) against the dp-1 masked run."""

import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from distributed_training_compare_jax_amd.config.schema import OptimConfig, TrainConfig, model_config_from_preset
from distributed_training_compare_jax_amd.data.synthetic import get_batch_iterator
from distributed_training_compare_jax_amd.models.reference import oracle_loss
from distributed_training_compare_jax_amd.ops import attention as A
from distributed_training_compare_jax_amd.parallel.dist import DistInfo, spawn
from distributed_training_compare_jax_amd.train.engine import Engine

pytestmark = pytest.mark.gpu

MODELS = {"hd64": dict(d_model=128, n_heads=2, n_layers=2, d_ff=256, max_seq_len=200),
          "hd128": dict(d_model=256, n_heads=2, n_layers=2, d_ff=512, max_seq_len=200)}
SEP = 7
LOSS_TOL, GRAD_TOL = 2e-2, 5e-2  # tests/test_engine_gpu.py test_model_grads_vs_oracle (bf16)


def _engine(dev, model, use_graph=False, doc=SEP, batch=4, steps=1, dropout=0.1, **kw):
    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=dropout, **MODELS[model])
    if doc is not None:
        kw["doc_mask_token"] = doc
    tc = TrainConfig(seed=0, parallel="dp", batch=batch, steps=steps, log_every=1, output_dir="/tmp/x",
                     use_graph=use_graph, **kw)
    return Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), DistInfo(0, 1, 0, dev, "nccl")), mc


ROWS = 16  # run_step: tokens per (micro)step a multiple of 64, as the grouped weight-gradient kernel asks (8 x 200)


def _batches(mc, n, rows=4, p=0.15):
    """Rows of ordinary ids with the separator at about every 7th position: frequent enough that the masked and the
    unmasked autograd oracle lie 1.3e-1 (2 heads of 64) and 8e-2 (2 heads of 128) apart on the first batch at the
    initial weights, four times LOSS_TOL and more (test_grads_vs_masked_oracle asserts the gap)."""
    g = np.random.default_rng(11)
    out = []
    for _ in range(n):
        b = g.integers(SEP + 1, 999, (rows, mc.max_seq_len + 1)).astype(np.int32)
        b[g.random(b.shape) < p] = SEP
        out.append(b)
    return out


@pytest.mark.parametrize("model", list(MODELS))
def test_grads_vs_masked_oracle(cuda, model):
    eng, mc = _engine(cuda, model)
    b = _batches(mc, 1)[0]
    eng.set_batch(b)
    st, T = eng.stage, mc.max_seq_len
    ctx = {}
    eng._doc_bounds_into(ctx, eng.ids)
    h = st.embed_forward(eng.ids, eng.opt.step_t, 0, ctx)
    h = st.stage_forward(h, 4, ctx)
    rec = A.last_launch()
    assert rec.path == "fwd_rows32_doc", rec
    loss = st.head_forward(h, eng.labels, 1 / (4 * T), ctx)
    dx, dxc = st.head_backward(ctx, 1 / (4 * T), 0.0)
    dx, dxc = st.stage_backward(ctx, dx, dxc, 0.0)
    assert A.last_launch().path in ("bwd_rows32_doc_merged", "bwd_rows32_doc_128")
    st.embed_backward(ctx, dx, eng.opt.step_t, 0.0)
    torch.cuda.synchronize()
    params = {n: eng.flat.p(n).detach().cpu().clone().requires_grad_(True) for n in eng.flat.slots}
    ids, lab = torch.from_numpy(b[:, :-1]).contiguous(), torch.from_numpy(b[:, 1:]).contiguous()
    lo = oracle_loss(mc, params, ids, lab, 0, 0, doc_mask_token=SEP)
    lo.backward()
    with torch.no_grad():
        plain = oracle_loss(mc, params, ids, lab, 0, 0).item()
    worst = []
    for n in eng.flat.slots:
        g, go = eng.flat.g(n).cpu(), params[n].grad
        worst.append((((g - go).norm() / (go.norm() + 1e-12)).item(), n))
    print(f"doc {model}: loss {loss.item():.6f} masked oracle {lo.item():.6f}; worst relative grad errors:",
          sorted(worst)[-5:])
    print(f"doc {model}: unmasked oracle {plain:.6f}, {abs(plain - lo.item()):.3e} from the masked one")
    assert abs(plain - lo.item()) > 3 * LOSS_TOL, "the two oracles are too close for this test to tell them apart"
    assert abs(loss.item() - lo.item()) < LOSS_TOL, (loss.item(), lo.item())
    assert abs(loss.item() - plain) > LOSS_TOL, f"the loss {loss.item()} is the unmasked oracle's {plain}: mask ignored"
    for err, n in worst:
        assert err < GRAD_TOL, f"{n}: relative grad error {err:.3e}"


@pytest.mark.parametrize("model", list(MODELS))
def test_graph_replay_determinism_and_accumulation(cuda, model):
    """Five steps: hipGraph replay equals eager bit for bit, two runs are equal bit for bit, grad_accum 2 follows
    grad_accum 1 to 1e-3 (tighter than the 2e-3 tests/test_grad_accum_gpu.py allows its accumulated bf16 steps;
    tests/test_engine_gpu.py, whose tolerances the other tests here mirror, has no accumulation case): every row's
    forward arithmetic is the same, the microsteps sum the loss and the weight
    gradients in another fp32 order (1e-6 on the first loss), and four bf16 parameter updates carry that on.  The
    same five steps without the mask give other losses, so the mask is not ignored."""
    def losses(**kw):
        eng, mc = _engine(cuda, model, steps=5, batch=ROWS, **kw)
        out = []
        for b in _batches(mc, 5, rows=ROWS):
            eng.set_batch(b)
            eng.run_step()
            out.append(eng.loss_value())
        return out, eng

    eager, _ = losses(use_graph=False)
    again, _ = losses(use_graph=False)
    graph, eng = losses(use_graph=True)
    assert eng.program.n_graphs >= 1
    assert eager == again, "two eager runs differ"
    assert graph == eager, "graph replay differs from eager"
    accum, _ = losses(use_graph=True, grad_accum=2)
    assert accum == pytest.approx(eager, rel=1e-3, abs=1e-3), (accum, eager)
    plain, _ = losses(use_graph=True, doc=-1)
    assert plain != eager, "the mask changed nothing"


def test_off_is_the_config_without_the_field(cuda):
    def run(doc):
        eng, mc = _engine(cuda, "hd64", use_graph=True, doc=doc, steps=5, batch=ROWS)
        it = get_batch_iterator(ROWS, mc.max_seq_len + 1, vocab=999)
        out = []
        for _ in range(5):
            eng.set_batch(next(it))
            eng.run_step()
            out.append(eng.loss_value())
        return out, eng.flat.p("wte").clone()

    (la, pa), (lb, pb) = run(-1), run(None)
    assert la == lb and torch.equal(pa, pb)


def test_evaluate_is_the_masked_training_forward(cuda):
    """One held-out batch: Engine.evaluate's loss is, bit for bit, the training forward's loss on the same rows under
    the same mask with dropout 0 (as tests/test_eval_engine_gpu.py holds the unmasked evaluation), and not the
    unmasked forward's.  The separator is the stream's most frequent token."""
    from dataclasses import replace

    from distributed_training_compare_jax_amd.data import synthetic
    from distributed_training_compare_jax_amd.models.gpt import full_forward_loss

    stream = synthetic.SyntheticTokenStream(vocab=999, seed=0)
    sep = int(stream.rank_to_id[0])
    eng, mc = _engine(cuda, "hd64", use_graph=False, doc=sep, batch=ROWS)
    eng.set_batch(next(get_batch_iterator(ROWS, mc.max_seq_len + 1, vocab=999)))
    eng.run_step()
    out = eng.evaluate(1)
    rows = synthetic.heldout_rows(stream, 0, 0, ROWS, ROWS, mc.max_seq_len + 1)
    ids, labels = (torch.from_numpy(rows[:, :-1]).contiguous().cuda(), torch.from_numpy(rows[:, 1:]).contiguous().cuda())
    assert int((ids == sep).sum()) >= ROWS, "the separator is too rare in the held-out batch to show anything"
    st = eng.stage
    cfg = st.cfg
    st.cfg = replace(cfg, dropout=0.0)
    try:
        masked, _ = full_forward_loss(st, ids, labels, eng.opt.step_t, ctx={"doc": A.doc_bounds(ids, sep)})
        plain, _ = full_forward_loss(st, ids, labels, eng.opt.step_t)
    finally:
        st.cfg = cfg
    torch.cuda.synchronize()
    assert out["loss"] == float(masked.item()), (out["loss"], float(masked.item()))
    assert out["loss"] != float(plain.item())


# ------------------------------------------------------------------------------------------ tp 2 over P2P
TP_STEPS = 5


def _tp_worker(parallel, kw, doc, out_dir):
    os.environ["DTC_DIST_BACKEND"] = "gloo"
    from distributed_training_compare_jax_amd.parallel.dist import destroy, init_distributed

    mc = model_config_from_preset("tiny", vocab_size=1000, dropout=0.1, **MODELS["hd64"])
    tc = TrainConfig(seed=0, parallel=parallel, batch=ROWS, steps=TP_STEPS, log_every=1000, output_dir="/tmp/unused",
                     device="cuda", warmup_steps=0, doc_mask_token=doc, **kw)
    d = init_distributed("cuda")
    eng = Engine(mc, tc, OptimConfig(lr=1e-3, weight_decay=0.1, grad_clip=1.0), d)
    losses, paths = [], set()
    for b in _batches(mc, TP_STEPS, rows=ROWS):
        eng.set_batch(b[eng.feed_row0:eng.feed_row0 + eng.feed_rows])
        eng.run_step()
        losses.append(eng.loss_value())
        paths.add(A.last_launch().path)
    torch.cuda.synchronize()
    eng.check_health()
    torch.save({"losses": losses, "paths": sorted(paths), "sp": eng.stage.sp, "heads": eng.stage.heads_local,
                "p2p": [n for n, _ in eng._live_transports()]}, os.path.join(out_dir, f"rank{d.rank}.pt"))
    eng.close()
    destroy()


@functools.lru_cache(maxsize=None)
def _tp_run(parallel, world, kw_items, doc):
    with tempfile.TemporaryDirectory() as td:
        if world == 1:
            for k in ("WORLD_SIZE", "RANK"):
                os.environ.pop(k, None)
            _tp_worker(parallel, dict(kw_items), doc, td)
        else:
            spawn(_tp_worker, world, args=(parallel, dict(kw_items), doc, td))
        return [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(world)]


@pytest.mark.slow
@pytest.mark.parametrize("sp", [False, True], ids=["tp2_p2p", "tp2_p2p_sp"])
def test_tp2_over_p2p_matches_dp1(cuda, sp):
    """Five masked steps on two TP ranks (one head each, in-graph P2P collectives) against the dp-1 masked run, at
    the tolerance the rig holds two ranks to a single GPU with (tests/test_dist_gpu.py
    test_two_ranks_match_single_gpu: 2e-2).  Every rank computes the bounds from the ids of all the rows its
    attention runs on and reaches the doc kernels; the unmasked dp-1 run is further away than that tolerance."""
    one = _tp_run("dp", 1, (), SEP)[0]
    plain = _tp_run("dp", 1, (), -1)[0]
    two = _tp_run("tp", 2, tuple(sorted(dict(tp_comm="p2p", tp_sequence_parallel=sp).items())), SEP)
    assert abs(plain["losses"][0] - one["losses"][0]) > 2 * 2e-2, (plain["losses"], one["losses"])
    for r in two:
        assert r["sp"] == sp and r["heads"] == 1 and "p2p" in r["p2p"]
        assert r["paths"] == ["bwd_rows32_doc_merged"], r["paths"]  # the step's last attention call
        assert r["losses"] == pytest.approx(one["losses"], rel=2e-2, abs=2e-2), (r["losses"], one["losses"])
    assert two[0]["losses"] == two[1]["losses"]
