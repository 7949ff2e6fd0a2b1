"""Configuration schema.

Mirrors the three frozen dataclasses of the reference (``config/schema.py:7-38``):
``ModelConfig``, ``OptimConfig`` and ``TrainConfig`` keep every reference field with
the same name and meaning, so the reference YAML files load unchanged.  New fields
are optional and default to the reference behaviour:

* ``ModelConfig.vocab_pad_multiple`` — the vocab is padded (masked pad logits) to a
  multiple of this so TP works at 4 and 8 GPUs (reference quirk: 50258 = 2*13*1933,
  ``parallel/sharding.py:35``).
* ``TrainConfig.dtype`` — ``bf16`` (MFMA bf16, fp32 master/accum) or ``fp32``.
* ``TrainConfig.dp/tp/pp`` — explicit mesh degrees for hybrid runs (reference: one
  1-D axis, ``train/train.py:29``).
* ``TrainConfig.pp_schedule`` (``gpipe`` | ``1f1b`` | ``zb``: 1F1B with the backward split into the
  input-gradient chain and the deferred weight gradients, the latter placed in the pipeline's idle gaps,
  ``parallel/pp.py``), ``pp_clip`` (``local`` is the
  reference's stage-local global-norm clip, ``create_train_step.py:190``; ``global``
  all-reduces the norm across stages).
* ``TrainConfig.data`` (``synthetic`` | ``fineweb``), ``use_graph``, ``profile`` (roctx
  ranges, device step times and a Chrome trace under ``<output_dir>/trace/``, see
  ``utils/trace.py``), ``watchdog_s`` (abort a rank whose step stalls that long, 0 = off),
  ``dp_bucket_mb`` / ``dp_tail_mb`` (DP grad bucket sizes, cut at layer boundaries and issued as
  soon as their last layer's grads are final; the last bucket is kept small because its
  all-reduce is exposed: for the reference model 98 / 48 / 48 / 36 / 12 MB), ``dp_embed_gather`` (DP: all-gather the embedding
  output grads and rebuild wte/wpe grads locally instead of all-reducing the 103 MB table),
  ``warmup_steps`` (reference hard-codes 5, ``train/train.py:64``), ``ckpt_every``/``resume``,
  ``tp_comm`` (``auto`` | ``p2p`` | ``rccl``: TP activation all-reduces as in-graph xGMI
  peer-to-peer kernels, ``parallel/p2p.py``; ``auto`` = p2p on a GPU RCCL group),
  ``defer_optimizer`` / ``defer_groups`` (run the non-embedding AdamW under the next step's
  forward in that many layer groups, on its own stream with a capped grid, ``DTC_DEFER_BLOCKS``;
  exact, off by default: measured slower at the reference size because the forward GEMMs run
  ~2x slower while the AdamW blocks share their CUs, ``profiles/r2_ab_defer_optimizer.log``),
  ``zero_stage`` (1 = ZeRO-1 Adam-state sharding over the DP group, ``ShardedAdamW``; pure DP only),
  ``wgrad_group`` (weight gradients deferred to grouped launches of that many layers, 0 = the whole
  stage plus the lm_head in one launch, -1 = each Dense's right after its dgrad; None = auto: 0 at
  dp = 1, 2 under DP so each group's buckets overlap the rest of the backward), ``pp_split``
  (``cost``: the contiguous layer split minimising the most expensive stage, counting lm_head + CE as
  ``pp_head_cost`` blocks on the last stage -- default from FLOPs, ``parallel/mesh.py``; ``even``: the
  remainder layers to the earliest stages), ``dp_grad_dtype`` / ``pp_comm_dtype`` / ``tp_comm_dtype`` (``bf16``: the DP
  gradient buckets / PP stage messages / TP partial sums travel as bf16 and are summed in fp32,
  ``ops/payload.py``, ``parallel/tp.py reduce_to``; the TP residual is added after the sum, unrounded),
  ``pp_comm`` (``rccl`` | ``p2p``: the PP stage messages, loss sum and ``pp_clip: global`` norm as eager
  process-group calls between graph segments, or as in-graph peer-to-peer kernels, ``parallel/p2p.py P2PPipe``:
  one hipGraph per stage step at dp = 1; GPU, pp <= 8, tp = 1; default ``rccl``),
  ``dp_comm`` (``rccl`` | ``p2p``: the DP gradient buckets, the loss sum and the embedding-gradient gather as
  process-group collectives, or as in-graph peer-to-peer kernels on one comm stream forked inside the step,
  ``parallel/p2p.py P2PGradReduce``: a pure-DP step is one hipGraph; GPU, 2 <= dp <= 8 or the dp = 1
  rehearsal, tp = pp = 1, zero_stage = 0; default ``rccl``),
  ``zero_comm`` (``rccl`` | ``p2p``, with ``zero_stage: 1``: ``ShardedAdamW``'s exposed process-group reduce-scatter
  and all-gather, or the DP buckets reduce-scattered under the backward, the AdamW on the owned slices and a
  per-bucket parameter gather that also writes the bf16 mirror, all in-graph peer-to-peer kernels,
  ``parallel/p2p.py P2PZeroShard`` + ``train/optimizer.py P2PShardedAdamW``: one hipGraph per step, ``dp_grad_dtype``
  honoured; GPU, 2 <= dp <= 8 or the dp = 1 rehearsal, tp = pp = 1, ``dp_comm: rccl``; default ``rccl``).
* ``TrainConfig.grad_accum`` (k, default 1): ``batch`` stays the global batch of ONE optimizer update; each rank's
  local rows run as k microbatches of ``b_local / k`` rows inside one step (one update, one loss, one CSV row), the
  gradients accumulated in place, so the peak activation memory is that of one microbatch.  Every DP / TP / ZeRO-1
  layout and transport (``train/engine.py``); pp > 1 accumulates through ``pp_microbatches`` instead.
* ``OptimConfig.lr_schedule`` (``constant`` | ``warmup_cosine`` | ``warmup_linear`` | ``wsd``) with ``lr_warmup_steps`` (W), ``lr_decay_steps``
  (N, warmup included) and ``lr_min_ratio`` (r): ``optax.warmup_cosine_decay_schedule(0, lr, W, N, lr * r)`` under
  ``scale_by_schedule``, evaluated on the device once per step from the step counter (``csrc/elementwise.hip``), so
  a captured step replays the schedule instead of one frozen rate; :meth:`OptimConfig.lr_at` is its float64 value.
  ``wsd`` (warmup, stable, decay) adds ``lr_cooldown_steps`` (C >= 1, W + C <= N): ``lr * c / W`` for c < W, ``lr``
  up to update N - C, ``lr * (1 - (1 - r) (c - (N - C)) / C)`` over the last C, ``lr * r`` from update N on (c = t - 1);
  ``warmup_linear`` is wsd with C = N - W, evaluated by the same arithmetic (the name ``linear`` is not accepted).
* ``OptimConfig.param_groups``: a list of ``{match: [fnmatch patterns on ParamSpec.name], weight_decay: x, lr_scale:
  s}`` (either value optional, not both missing), normalised to a tuple of frozen :class:`ParamGroup` records.  The
  first group that matches a parameter gives it its decay (in place of the global one) and multiplies its scheduled
  rate by ``lr_scale``; unmatched parameters keep the global decay and scale 1.  Unknown keys, an empty ``match``,
  negative or non-finite values raise ``ValueError``; the engine also refuses a pattern that matches no parameter
  of the model.  The groups live inside the fused AdamW kernels (``ops/optim.py GroupTable``); a checkpoint records
  :meth:`OptimConfig.groups_key` ('' without groups).
* ``TrainConfig.eval_every`` (default 0 = off) / ``eval_batches`` (default 8): every ``eval_every`` optimizer updates and
  after the last one, a forward-only pass over ``eval_batches`` held-out batches of ``batch`` rows (the synthetic
  stream read from ``data/synthetic.py EVAL_POS_BASE`` on: the same tokens at every evaluation and under every
  layout) reports mean loss, perplexity and top-1 accuracy: one console line, ``eval.csv`` beside ``log.csv``,
  ``eval_last`` / ``eval_time_total_s`` in ``metrics.json``.  Its own hipGraph, dropout 0, the training forward's
  kernels with a lm_head epilogue that stores no logits (``train/engine.py Engine.evaluate``); the training run is bit
  for bit the one without it, and its clock stops for the duration.  pp = 1; not with ``defer_optimizer`` (parameters
  are not final between steps) or ``data: fineweb``.
* ``TrainConfig.doc_mask_token`` (default -1 = off): the id of the separator token of packed rows.  Attention then
  stops at document boundaries (a document starts at position 0 and after every separator; positions stay absolute,
  the loss is unchanged), in training and in evaluation, with bounds computed inside the step program from each
  (micro)step's ids.  GPU: bf16 at head_dim 64 / 128, pp = 1; ``metrics.json`` records the value.
"""

from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field, replace
from typing import Any, Dict, Optional, Tuple

PyTree = Any

# GPT-2 BPE (50257) + the added <pad> token (reference data/fineweb_edu.py:8-12, main.py:17-18).
REFERENCE_VOCAB_SIZE = 50258


@dataclass(frozen=True)
class ModelConfig:
    vocab_size: int
    d_model: int
    n_layers: int
    n_heads: int
    d_ff: int
    max_seq_len: int
    dropout: float
    parallel: str = "none"
    # --- extensions (defaults = reference behaviour) ---
    vocab_pad_multiple: int = 128
    layernorm_eps: float = 1e-6  # flax nn.LayerNorm default
    name: str = "gpt-ref-89M"

    @property
    def head_dim(self) -> int:
        return self.d_model // self.n_heads

    @property
    def padded_vocab(self) -> int:
        m = max(1, int(self.vocab_pad_multiple))
        return ((self.vocab_size + m - 1) // m) * m

    def num_params(self) -> int:
        """Parameter count of the reference architecture (unpadded vocab)."""
        D, F, V, T, L = self.d_model, self.d_ff, self.vocab_size, self.max_seq_len, self.n_layers
        per_layer = 4 * D * D + 4 * D + D * F + F + F * D + D + 4 * D
        return V * D + T * D + L * per_layer + 2 * D + D * V + V

    def flops_per_token(self, causal: bool = True) -> float:
        """Matmul FLOPs per token, fwd+bwd: 6 * N_matmul + attention.  ``causal`` (default): the useful
        work of the causal attention, (T + 1) / 2 keys per query on average; ``causal=False``: the full
        T x T count SURVEY §2.4 / BASELINE.md's 1.715 TFLOP/step estimate use."""
        D, F, V, T, L = self.d_model, self.d_ff, self.vocab_size, self.max_seq_len, self.n_layers
        mm = L * (4 * D * D + 2 * D * F) + D * V
        keys = (T + 1) / 2.0 if causal else float(T)
        attn = L * 2 * keys * D  # QK^T + PV multiply-adds per token
        return 6.0 * mm + 3.0 * 2.0 * attn


_SCHEDULES = ("constant", "warmup_cosine", "warmup_linear", "wsd")


@dataclass(frozen=True)
class ParamGroup:
    """One entry of ``OptimConfig.param_groups``: the parameters whose name matches any ``match`` pattern (fnmatch on
    ``ParamSpec.name``) take ``weight_decay`` in place of the global one and ``lr_scale`` times the (scheduled)
    rate; None = the default (the global decay, scale 1)."""
    match: Tuple[str, ...]
    weight_decay: Optional[float] = None
    lr_scale: Optional[float] = None

    def matches(self, name: str) -> bool:
        import fnmatch

        return any(fnmatch.fnmatchcase(name, pat) for pat in self.match)


def _param_group(i: int, g) -> ParamGroup:
    import math

    if isinstance(g, ParamGroup):
        g = dict(match=g.match, weight_decay=g.weight_decay, lr_scale=g.lr_scale)
    if not isinstance(g, dict):
        raise ValueError(f"param_groups[{i}]={g!r}: expected a mapping with 'match' and 'weight_decay' / 'lr_scale'")
    unknown = sorted(set(g) - {"match", "weight_decay", "lr_scale"})
    if unknown:
        raise ValueError(f"param_groups[{i}]: unknown key {unknown[0]!r} (expected match, weight_decay, lr_scale)")
    match = g.get("match")
    if isinstance(match, str):
        match = [match]
    if not match or not all(isinstance(m, str) and m for m in match):
        raise ValueError(f"param_groups[{i}]: match={g.get('match')!r}: expected a non-empty list of name patterns")
    vals = {}
    for k in ("weight_decay", "lr_scale"):
        v = g.get(k)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"param_groups[{i}]: {k}={v!r}: expected a finite number >= 0")
            v = float(v)
        vals[k] = v
    if vals["weight_decay"] is None and vals["lr_scale"] is None:
        raise ValueError(f"param_groups[{i}] (match={list(match)!r}) sets neither weight_decay nor lr_scale")
    return ParamGroup(tuple(match), vals["weight_decay"], vals["lr_scale"])


@dataclass(frozen=True)
class OptimConfig:
    lr: float
    weight_decay: float
    grad_clip: float
    # optax.adamw defaults (optax 0.2.6)
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    # --- extensions (defaults = reference behaviour: one constant rate) ---
    lr_schedule: str = "constant"  # constant | warmup_cosine | warmup_linear | wsd
    lr_warmup_steps: int = 0       # W: linear warmup from 0 over the first W updates
    lr_decay_steps: int = 0        # N: the decay reaches lr * lr_min_ratio at update N (warmup included)
    lr_min_ratio: float = 0.0      # r: the floor as a fraction of lr
    lr_cooldown_steps: int = 0     # C (wsd): the linear decay covers the last C of the N updates
    # parameter groups: [{match: [patterns], weight_decay: .., lr_scale: ..}], first match wins (ParamGroup)
    param_groups: Tuple[ParamGroup, ...] = ()

    def __post_init__(self):
        if self.lr_schedule not in _SCHEDULES:
            raise ValueError(f"lr_schedule={self.lr_schedule!r}: expected one of {', '.join(map(repr, _SCHEDULES))}")
        W, N, r, C = self.lr_warmup_steps, self.lr_decay_steps, self.lr_min_ratio, self.lr_cooldown_steps
        if isinstance(W, bool) or isinstance(N, bool) or int(W) != W or int(N) != N or W < 0 or N < 0:
            raise ValueError(f"lr_warmup_steps={W!r}, lr_decay_steps={N!r}: expected non-negative integers")
        if isinstance(C, bool) or not isinstance(C, int) or C < 0:
            raise ValueError(f"lr_cooldown_steps={C!r}: expected a non-negative integer")
        if not (0.0 <= float(r) <= 1.0):
            raise ValueError(f"lr_min_ratio={r!r}: expected a ratio in [0, 1]")
        if self.lr_schedule in ("warmup_cosine", "warmup_linear") and N <= W:
            raise ValueError(f"lr_schedule={self.lr_schedule} needs lr_decay_steps > lr_warmup_steps (got N={N}, "
                             f"W={W}: N counts the warmup)")
        if self.lr_schedule == "wsd" and (C < 1 or W + C > N):
            raise ValueError(f"lr_schedule=wsd needs lr_cooldown_steps >= 1 and lr_warmup_steps + lr_cooldown_steps <= "
                             f"lr_decay_steps (got W={W}, C={C}, N={N})")
        groups = self.param_groups
        if groups is None:
            groups = ()
        if isinstance(groups, (dict, str, ParamGroup)) or not isinstance(groups, (list, tuple)):
            raise ValueError(f"param_groups={groups!r}: expected a list of mappings")
        object.__setattr__(self, "param_groups", tuple(_param_group(i, g) for i, g in enumerate(groups)))

    @property
    def scheduled(self) -> bool:
        return self.lr_schedule != "constant"

    @property
    def cooldown(self) -> int:
        """C of the linear-decay schedules: ``lr_cooldown_steps`` for wsd, N - W for warmup_linear (which IS wsd with
        that C: one arithmetic on the host and on the device)."""
        if self.lr_schedule == "warmup_linear":
            return int(self.lr_decay_steps) - int(self.lr_warmup_steps)
        return int(self.lr_cooldown_steps) if self.lr_schedule == "wsd" else 0

    def lr_at(self, t: int) -> float:
        """The learning rate of update ``t`` (1-based: the already-incremented step counter) in float64.  optax
        counts the updates already applied, c = t - 1: lr * c / W during warmup, then either the cosine from lr down
        to lr * r over the N - W steps that follow, or (wsd; warmup_linear = wsd with C = N - W) lr up to update
        N - C and a straight line down to lr * r over the last C; lr * r from update N on."""
        import math

        if not self.scheduled:
            return float(self.lr)
        W, N, r = int(self.lr_warmup_steps), int(self.lr_decay_steps), float(self.lr_min_ratio)
        c = int(t) - 1
        if c < W:
            return float(self.lr) * c / W
        if self.lr_schedule in ("wsd", "warmup_linear"):
            C = self.cooldown
            if c < N - C:
                return float(self.lr)
            if c >= N:
                return float(self.lr) * r
            return float(self.lr) * (1.0 - (1.0 - r) * (c - (N - C)) / C)
        x = min(c - W, N - W) / (N - W)
        return float(self.lr) * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * x)))

    def schedule_key(self) -> str:
        """What a checkpoint records so that a resume under other schedule fields is refused (the cooldown only for
        the kinds that have one: the strings of constant and warmup_cosine are those of older checkpoints)."""
        key = (f"{self.lr_schedule}:{int(self.lr_warmup_steps)}:{int(self.lr_decay_steps)}:"
               f"{float(self.lr_min_ratio)!r}")
        return f"{key}:{self.cooldown}" if self.lr_schedule in ("wsd", "warmup_linear") else key

    # -- parameter groups ---------------------------------------------------------
    def group_of(self, name: str) -> int:
        """Index of the first group whose patterns match ``name``, or -1 (the global decay, scale 1)."""
        for i, g in enumerate(self.param_groups):
            if g.matches(name):
                return i
        return -1

    def group_values(self, name: str) -> Tuple[float, float]:
        """(weight_decay, lr_scale) of the parameter ``name``."""
        i = self.group_of(name)
        if i < 0:
            return float(self.weight_decay), 1.0
        g = self.param_groups[i]
        return (float(self.weight_decay) if g.weight_decay is None else g.weight_decay,
                1.0 if g.lr_scale is None else g.lr_scale)

    def check_groups(self, names) -> None:
        """Every pattern must match at least one of ``names`` (the whole model's parameter names): a typo would
        otherwise silently leave its parameters in the default group."""
        names = list(names)
        for i, g in enumerate(self.param_groups):
            for pat in g.match:
                if not any(ParamGroup((pat,), 0.0).matches(n) for n in names):
                    raise ValueError(f"param_groups[{i}]: pattern {pat!r} matches no parameter (names look like "
                                     f"{', '.join(names[:4])}, ...)")

    def groups_key(self) -> str:
        """What a checkpoint records so that a resume under other groups is refused; '' when none is configured."""
        return ";".join(f"{','.join(g.match)}|wd={g.weight_decay!r}|s={g.lr_scale!r}" for g in self.param_groups)


@dataclass(frozen=True)
class TrainConfig:
    seed: int
    parallel: str
    # batching
    batch: int
    # steps
    steps: int
    log_every: int
    # output
    output_dir: str
    # pipeline parallelism
    pp_microbatches: int = 1
    # --- extensions ---
    # gradient accumulation (pp == 1): each rank's local batch as grad_accum microbatches inside one step; `batch`
    # stays the global batch of one optimizer update (train/engine.py)
    grad_accum: int = 1
    dtype: str = "bf16"
    # bf16 | fp8 | mxfp8: the forward qkv / out_proj / fc1 / fc2 GEMMs.  fp8 = e4m3 operands with per-tensor
    # power-of-two scales from the current tensor (ops/fp8.py); mxfp8 = e4m3 operands with one power-of-two scale per
    # 32 elements of k (OCP microscaling, ops/mxfp8.py), quantised inside the LayerNorm and GELU kernels that produce
    # them; the backward, the lm_head and everything else stay as they are
    fwd_gemm_dtype: str = "bf16"
    dp: Optional[int] = None
    tp: Optional[int] = None
    pp: Optional[int] = None
    pp_schedule: str = "gpipe"
    pp_clip: str = "local"
    data: str = "synthetic"
    use_graph: bool = True
    profile: bool = False
    watchdog_s: float = 900.0
    tp_comm: str = "auto"
    defer_optimizer: bool = False
    defer_groups: int = 4
    dp_bucket_mb: float = 40.0
    dp_tail_mb: float = 16.0
    dp_embed_gather: bool = True
    zero_stage: int = 0  # 1 = ZeRO-1: Adam state sharded over the DP group (train/optimizer.py)
    wgrad_group: Optional[int] = None  # deferred grouped weight gradients (models/gpt.py set_wgrad_group)
    pp_split: str = "cost"  # cost | even: PP layer split (parallel/mesh.py split_layers)
    dp_grad_dtype: str = "fp32"  # fp32 | bf16: DP gradient payload (bf16: all-to-all + fp32 shard sums)
    # fp32 | bf16 | auto: PP activation / gradient messages; auto = bf16 when the compute dtype is bf16 (5000-step
    # pp2 curve: the same gap to dp1 as fp32 messages; half the bytes of the latency-bound pp8 hops)
    pp_comm_dtype: str = "auto"
    # rccl | p2p: how the PP stage messages, the PP loss sum and the pp_clip: global norm travel.  rccl = eager
    # send/recv and all-reduces between graph segments (a cut per message exchange); p2p = stream-ordered kernels
    # over IPC-mapped peer buffers (parallel/p2p.py P2PPipe), so a stage's step at dp == 1 is ONE hipGraph with no
    # eager collective.  GPU only, 2 <= pp <= 8, tp == 1.  No auto: the default stays rccl until p2p has run across
    # real GPUs (docs/CAPTURE.md)
    pp_comm: str = "rccl"
    # rccl | p2p: how the DP gradient buckets, the DP loss sum and the embedding-output gradient gather travel.
    # rccl = process-group collectives (cut out of the graph at world > 1; the bf16 payload chain always);
    # p2p = stream-ordered kernels over IPC-mapped peer buffers (parallel/p2p.py P2PGradReduce) on one comm stream
    # forked inside the step, so a pure-DP step is ONE hipGraph with no eager collective.  GPU only, tp == pp == 1,
    # zero_stage == 0, 2 <= dp <= 8 (dp == 1 only with dp_comm_rehearsal).  No auto: the default stays rccl until
    # p2p has run across real GPUs (docs/CAPTURE.md)
    dp_comm: str = "rccl"
    # rccl | p2p: the transport of the SHARDED optimizer step (zero_stage: 1; dp_comm names that of the replicated
    # one and stays rccl).  rccl = ShardedAdamW: one reduce-scatter after the backward and one all-gather after the
    # update through the process group, both exposed, then a full fp32 -> bf16 mirror cast.  p2p = the gradient
    # buckets reduce-scattered under the backward as stream-ordered kernels over IPC-mapped peer buffers
    # (parallel/p2p.py P2PZeroShard), AdamW on the owned slices (train/optimizer.py P2PShardedAdamW), per-bucket
    # parameter gathers that write the bf16 mirror in the same pass: ONE hipGraph per step, no eager collective,
    # dp_grad_dtype honoured.  GPU only, tp == pp == 1, 2 <= dp <= 8 (dp == 1 only with dp_comm_rehearsal).  No
    # auto: the default stays rccl until p2p has run across real GPUs (docs/CAPTURE.md)
    zero_comm: str = "rccl"
    # fp32 | bf16 | auto: TP row-parallel / input-gradient partials (fp32 sums either way); auto = bf16 when the
    # compute dtype is bf16 (5000-step tp2 curve: the same gap to dp1 as fp32, profiles/r5_cross_strategy.md)
    tp_comm_dtype: str = "auto"
    # Megatron-style sequence parallelism over the TP group (pp == 1, batch % tp == 0): the residual stream,
    # LayerNorms and embedding output on batch/tp sequences per rank; reduce-scatter + all-gather in place of
    # each TP all-reduce (models/gpt.py enable_sequence_parallel).  None = auto: on whenever it applies
    tp_sequence_parallel: Optional[bool] = None
    pp_head_cost: Optional[float] = None  # lm_head + CE in blocks (None: parallel/mesh.py head_cost_blocks)
    # lm_head + CE split by vocab over the last two pipeline stages (1f1b / zb, tp == 1; parallel/pp.py
    # _head_split).  None = auto: on when the head alone outweighs an even share of the model (pp >= 4)
    pp_head_split: Optional[bool] = None
    warmup_steps: int = 5
    ckpt_every: int = 0
    resume: bool = False
    deterministic: bool = False
    # DP collective rehearsal: at dp == 1 on an initialised (one-rank) process group, run the DP code path
    # anyway -- bucket all-reduces, embedding-grad all-gather, loss all-reduce, ZeRO-1 reduce-scatter /
    # all-gather, bf16 all-to-all payloads -- on a one-member communicator (identities: same math as dp1).
    # The one-GPU box uses it to execute the exact RCCL call sequence of a DP step (tests/test_rccl_gpu.py)
    dp_comm_rehearsal: bool = False
    # capture the step's collectives INTO its hipGraph (one graph per step) instead of cutting the graph at
    # each collective and issuing it eagerly between segments (parallel/program.py).  None = auto: on for a
    # ONE-rank RCCL process group (the rehearsal, where it was measured: 11.39-11.41 ms/step captured vs
    # 11.62-11.64 cut, profiles/r5_rccl_rehearsal.md), off at world > 1 until capture has run against real
    # peers (docs/CAPTURE.md), off for gloo; DTC_CAPTURE_COMMS=1 / 0 force it
    capture_comms: Optional[bool] = None
    device: str = "auto"  # auto | cuda | cpu
    batch_is_global: bool = True  # reference: `batch` is the global batch
    # held-out evaluation (train/engine.py Engine.evaluate): every eval_every optimizer updates and after the last
    # one, a forward-only pass over eval_batches held-out batches of `batch` rows -> loss, perplexity, top-1.  0 = off
    eval_every: int = 0
    eval_batches: int = 8
    # document-masked attention for packed rows: the id of the separator (end-of-text) token.  Position t starts a
    # document iff t == 0 or ids[t-1] is the separator, and a query sees only the keys of its own document
    # (ops/attention.py doc_bounds; the separator belongs to the document it ends).  Position embeddings stay
    # absolute and the loss is unchanged.  -1 = off: nothing is allocated or launched.  GPU: bf16, head_dim 64 / 128,
    # pp == 1 (train/engine.py refuses the rest by name)
    doc_mask_token: int = -1

    def __post_init__(self):
        if isinstance(self.doc_mask_token, bool) or not isinstance(self.doc_mask_token, int) or self.doc_mask_token < -1:
            raise ValueError(f"doc_mask_token={self.doc_mask_token!r}: expected a token id >= 0, or -1 (off)")
        for name in ("eval_every", "eval_batches"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name}={v!r}: expected a non-negative integer")
        if self.eval_every > 0:
            if self.eval_batches < 1:
                raise ValueError(f"eval_every={self.eval_every} needs eval_batches >= 1 (got {self.eval_batches})")
            if self.defer_optimizer:
                raise ValueError("eval_every > 0 cannot be combined with defer_optimizer=true (the deferred update "
                                 "runs under the next step's forward: parameters are not final between steps)")
            if (self.pp or 1) > 1:  # (parallel: pp resolves to the world size: refused by the engine)
                raise ValueError("eval_every > 0 needs pp == 1: evaluation under pipeline parallelism is not "
                                 "implemented (the follow-up: a forward-only pipeline schedule)")
            if self.data != "synthetic":
                raise ValueError(f"eval_every > 0 with data={self.data!r}: the held-out set is defined for the "
                                 "synthetic stream only (data: synthetic)")


# Named model presets.  "ref" is the reference's configs/model_config.yaml.
MODEL_PRESETS: Dict[str, Dict[str, Any]] = {
    "ref": dict(d_model=512, n_layers=12, n_heads=16, d_ff=2048, max_seq_len=512, dropout=0.1,
                name="gpt-ref-89M"),
    "gpt2-small": dict(d_model=768, n_layers=12, n_heads=12, d_ff=3072, max_seq_len=1024, dropout=0.1,
                       name="gpt2-small-124M"),
    "gpt2-medium": dict(d_model=1024, n_layers=24, n_heads=16, d_ff=4096, max_seq_len=1024, dropout=0.1,
                        name="gpt2-medium-355M"),
    # GPT-3 XL's shape with 16 heads of 128 (the wide LayerNorm kernels + head_dim 128 attention)
    "gpt-1.3b": dict(d_model=2048, n_layers=24, n_heads=16, d_ff=8192, max_seq_len=2048, dropout=0.1,
                     name="gpt-1.3b"),
    "tiny": dict(d_model=64, n_layers=2, n_heads=2, d_ff=256, max_seq_len=64, dropout=0.1, name="tiny"),
}


def model_config_from_preset(preset: str, vocab_size: int = REFERENCE_VOCAB_SIZE, **overrides) -> ModelConfig:
    d = dict(MODEL_PRESETS[preset])
    d.update(overrides)
    return ModelConfig(vocab_size=vocab_size, **d)


def _filter_fields(cls, d: Dict[str, Any]) -> Dict[str, Any]:
    names = {f.name for f in dataclasses.fields(cls)}
    unknown = set(d) - names
    if unknown:
        raise TypeError(f"{cls.__name__}: unknown config keys {sorted(unknown)}")
    return d


def load_yaml(path: str) -> Dict[str, Any]:
    import yaml

    with open(path) as f:
        return yaml.safe_load(f) or {}


def build_configs(train_config_path: str, model_config_path: str = "configs/model_config.yaml",
                  optim_config_path: str = "configs/optim_config.yaml",
                  vocab_size: int = REFERENCE_VOCAB_SIZE):
    """Same assembly as reference main.py:14-30: vocab injected, parallel copied into ModelConfig."""
    mdict = load_yaml(model_config_path)
    mdict["vocab_size"] = vocab_size
    tdict = load_yaml(train_config_path)
    train_config = TrainConfig(**_filter_fields(TrainConfig, tdict))
    mdict["parallel"] = train_config.parallel
    model_config = ModelConfig(**_filter_fields(ModelConfig, mdict))
    opt_config = OptimConfig(**_filter_fields(OptimConfig, load_yaml(optim_config_path)))
    return train_config, model_config, opt_config


__all__ = [
    "PyTree", "ModelConfig", "OptimConfig", "ParamGroup", "TrainConfig", "MODEL_PRESETS", "REFERENCE_VOCAB_SIZE",
    "model_config_from_preset", "build_configs", "load_yaml", "replace", "field",
]
