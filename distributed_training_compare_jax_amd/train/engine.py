"""Training engine: one rank's model shard, flat buffers, optimizer and the step program.

Reference counterparts: the DP/TP jitted step (``train/create_train_step.py:24-52``), the
PP pmap/scan step (``:55-195``) and the state plumbing of ``train/train.py:22-233``.
One class serves every layout (DP, TP, PP and their products): the mesh decides which
layers/params this rank owns and which collectives run; the step itself is a static
sequence of HIP kernels + RCCL calls that :class:`StepProgram` captures into hipGraph
segments after the first eager warmup step.
"""

from __future__ import annotations

import math
import os
import warnings
from dataclasses import replace
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from ..config.schema import ModelConfig, OptimConfig, TrainConfig
from ..models.gpt import GPTStage, StageLayout
from ..models.params import stage_param_specs
from ..ops import attention as A
from ..ops import embedding as E
from ..ops import gemm as G
from ..ops import optim as O
from ..parallel.buffers import FlatParams
from ..parallel.dist import DistInfo
from ..parallel.dp import GradBuckets
from ..parallel.mesh import Mesh, build_mesh, head_cost_blocks, resolve_degrees, split_layers
from ..parallel.program import StepProgram, csig
from ..parallel.tp import TPComm
from .optimizer import FusedAdamW, P2PShardedAdamW, ShardedAdamW


class Engine:
    def __init__(self, model_cfg: ModelConfig, train_cfg: TrainConfig, opt_cfg: OptimConfig, dinfo: DistInfo):
        self.mcfg, self.tcfg, self.ocfg = model_cfg, train_cfg, opt_cfg
        self.dinfo = dinfo
        self.device = dinfo.device
        dp, tp, pp = resolve_degrees(train_cfg.parallel, dinfo.world, train_cfg.dp, train_cfg.tp, train_cfg.pp)
        # param_groups: every pattern must name a parameter of the WHOLE model (a stage holds only some), checked
        # here, before any collective, so every rank raises alike on a typo
        if opt_cfg.param_groups:
            from ..models.params import all_param_specs

            opt_cfg.check_groups([sp.name for sp in all_param_specs(model_cfg)])
        # pp_comm: p2p (the stage messages, the PP loss sum and the pp_clip: global norm as in-graph kernels over
        # IPC-mapped buffers, parallel/p2p.py P2PPipe): what it does not cover is refused here, before any collective
        if train_cfg.pp_comm not in ("rccl", "p2p"):
            raise ValueError(f"pp_comm={train_cfg.pp_comm!r}: expected 'rccl' or 'p2p'")
        if train_cfg.pp_comm == "p2p":
            why = None
            if pp == 1:
                why = "pp == 1 (there are no stage messages)"
            elif dinfo.device.type != "cuda":
                why = "a CPU device (the transport is HIP kernels over IPC-mapped device buffers)"
            elif pp > 8:
                why = f"pp={pp} (the peer buffers span one xGMI hive: at most 8 stages)"
            elif tp > 1:
                why = f"tp={tp} (out of scope: the TP and the PP peer buffers have not been run together; use tp = 1)"
            if why:
                raise ValueError(f"pp_comm: p2p cannot be combined with {why}")
        # zero_comm: p2p (ZeRO-1 as in-graph kernels on one peer object, parallel/p2p.py P2PZeroShard: per-bucket
        # reduce-scatters under the backward, the sharded AdamW, per-bucket parameter gathers): refused likewise, before
        # the dp_comm checks so that both fields set to p2p are answered under this one
        if train_cfg.zero_comm not in ("rccl", "p2p"):
            raise ValueError(f"zero_comm={train_cfg.zero_comm!r}: expected 'rccl' or 'p2p'")
        if train_cfg.zero_comm == "p2p":
            why = None
            if train_cfg.zero_stage != 1:
                why = f"zero_stage={train_cfg.zero_stage} (it names the transport of the sharded optimizer: zero_stage: 1)"
            elif dinfo.device.type != "cuda":
                why = "a CPU device (the transport is HIP kernels over IPC-mapped device buffers)"
            elif tp > 1:
                why = f"tp={tp} (ZeRO-1 is implemented for pure data parallelism; use tp = 1)"
            elif pp > 1:
                why = f"pp={pp} (ZeRO-1 is implemented for pure data parallelism; use pp = 1)"
            elif train_cfg.dp_comm == "p2p":
                why = ("dp_comm: p2p (that names the transport of the replicated-optimizer step; under zero_comm: p2p "
                       "the loss sum rides the ZeRO peer object: leave dp_comm at rccl)")
            elif dp > 8:
                why = f"dp={dp} (the peer buffers span one xGMI hive: at most 8 replicas)"
            elif dp == 1 and not train_cfg.dp_comm_rehearsal:
                why = "dp == 1 (there is nothing to shard; dp_comm_rehearsal: true runs the transport at world 1)"
            elif dp == 1 and not (dist.is_available() and dist.is_initialized()):
                why = "dp == 1 without a process group (the rehearsal needs one for the init handshake)"
            elif train_cfg.dtype not in ("bf16", "fp32"):
                why = f"dtype={train_cfg.dtype!r} (bf16 or fp32)"
            if why:
                raise ValueError(f"zero_comm: p2p cannot be combined with {why}")
        # dp_comm: p2p (the gradient buckets, the loss sum and the embedding-gradient gather of a pure-DP step as
        # in-graph kernels on one peer object, parallel/p2p.py P2PGradReduce): refused likewise, before any collective
        if train_cfg.dp_comm not in ("rccl", "p2p"):
            raise ValueError(f"dp_comm={train_cfg.dp_comm!r}: expected 'rccl' or 'p2p'")
        if train_cfg.dp_comm == "p2p":
            why = None
            if dinfo.device.type != "cuda":
                why = "a CPU device (the transport is HIP kernels over IPC-mapped device buffers)"
            elif tp > 1:
                why = f"tp={tp} (out of scope: the TP and the DP peer buffers have not been run together; use tp = 1)"
            elif pp > 1:
                why = f"pp={pp} (out of scope: the PP and the DP peer buffers have not been run together; use pp = 1)"
            elif train_cfg.zero_stage == 1:
                why = ("zero_stage=1 (out of scope: ShardedAdamW reduce-scatters through the process group; the "
                       "in-graph ZeRO-1 is zero_comm: p2p, with dp_comm left at rccl)")
            elif dp > 8:
                why = f"dp={dp} (the peer buffers span one xGMI hive: at most 8 replicas)"
            elif dp == 1 and not train_cfg.dp_comm_rehearsal:
                why = "dp == 1 (there is nothing to reduce; dp_comm_rehearsal: true runs the transport at world 1)"
            elif dp == 1 and not (dist.is_available() and dist.is_initialized()):
                why = "dp == 1 without a process group (the rehearsal needs one for the init handshake)"
            if why:
                raise ValueError(f"dp_comm: p2p cannot be combined with {why}")
        # grad_accum: k (the local batch as k microbatches inside one step, gradients accumulated in place): refused
        # here, by name, what it does not cover
        k_acc = train_cfg.grad_accum
        if isinstance(k_acc, bool) or not isinstance(k_acc, int) or k_acc < 1:
            raise ValueError(f"grad_accum={k_acc!r}: expected an integer >= 1")
        if k_acc > 1:
            why = None
            if pp > 1:
                why = (f"pp={pp} (a pipeline accumulates its own microbatches: set pp_microbatches, "
                       "and leave grad_accum at 1)")
            elif train_cfg.defer_optimizer:
                why = ("defer_optimizer=true (the deferred update is launched under the first forward of the next "
                       "step; it has not been run with more than one forward per step)")
            elif train_cfg.batch % dp == 0 and (train_cfg.batch // dp) % k_acc:
                why = (f"a local batch of {train_cfg.batch // dp} rows (batch {train_cfg.batch} / dp {dp}): it must "
                       f"split into {k_acc} whole microbatches")
            if why:
                raise ValueError(f"grad_accum={k_acc} cannot be combined with {why}")
        self.grad_accum = int(k_acc)
        # doc_mask_token: attention that stops at document boundaries (ops/attention.py doc_bounds; the bounds are
        # computed from each (micro)step's own ids inside the step program).  Tensor parallelism needs nothing: the
        # bounds depend on the row alone and every TP rank holds the ids of all the rows its attention runs on, with
        # and without sequence parallelism (self.ids is the whole local batch; sequence parallelism splits rows
        # only between the attention calls).  What it does not cover is refused here, by name.
        self.doc_token = int(train_cfg.doc_mask_token)
        if self.doc_token >= 0:
            why = None
            hd = model_cfg.d_model // model_cfg.n_heads
            if pp > 1:
                why = (f"pp={pp} (pipeline parallelism: the later stages hold no ids; the follow-up ships the bounds "
                       "with the stage message)")
            elif dinfo.device.type == "cuda" and train_cfg.dtype == "fp32":
                why = "dtype=fp32 on the GPU (the exact-fp32 attention kernels have no document mask; use bf16)"
            elif dinfo.device.type == "cuda" and hd not in (64, 128):
                why = (f"head_dim {hd} on the GPU (d_model {model_cfg.d_model} / n_heads {model_cfg.n_heads}): the "
                       "document-masked kernels are the 32-row family, head_dim 64 or 128")
            if why:
                raise ValueError(f"doc_mask_token={self.doc_token} cannot be combined with {why}")
        # eval_every: the held-out evaluation (evaluate) -- what it does not cover is refused here, by name
        if train_cfg.eval_every > 0:
            if pp > 1:
                raise ValueError(f"eval_every > 0 cannot be combined with pp={pp}: evaluation under pipeline parallelism "
                                 "is not implemented (the follow-up: a forward-only pipeline schedule)")
            from ..data.synthetic import check_heldout_disjoint

            # (a resumed run adds its earlier steps: train/loop.py checks again with the checkpoint's step)
            check_heldout_disjoint(train_cfg.warmup_steps + train_cfg.steps, train_cfg.batch, model_cfg.max_seq_len + 1)
        # lm_head + CE split by vocab over the last two pipeline stages (models/gpt.py head_split_*): auto when
        # the head alone outweighs an even share of the model (GPT-2 small at pp >= 5: 2.9 blocks vs 14.9 / pp)
        hsplit = train_cfg.pp_head_split
        hc_auto = head_cost_blocks(model_cfg) if train_cfg.pp_head_cost is None else float(train_cfg.pp_head_cost)
        if hsplit is None:
            hsplit = (pp >= 4 and tp == 1 and train_cfg.pp_schedule in ("1f1b", "zb")
                      and hc_auto > (model_cfg.n_layers + hc_auto) / pp)
        if hsplit and (pp < 2 or train_cfg.pp_schedule not in ("1f1b", "zb") or tp > 1):
            raise ValueError("pp_head_split needs pp >= 2, tp == 1 and the 1f1b or zb schedule")
        self.pp_head_split = bool(hsplit)
        if self.pp_head_split and model_cfg.padded_vocab % 128:
            # each half a multiple of 64 columns
            model_cfg = replace(model_cfg, vocab_pad_multiple=math.lcm(max(1, int(model_cfg.vocab_pad_multiple)), 128))
            self.mcfg = model_cfg
        if tp > 1:
            # every TP rank's vocab shard a multiple of 64 columns (the GEMM K-steps of the lm_head dgrad and
            # the 64-wide CE tiles): pad the vocab to a multiple of 64 * tp (GPT-2 at tp = 8: 50688 instead
            # of 50304 = 8 x 6288).  Pad rows are zero and masked, and the valid rows' canonical init does not
            # depend on the padded length, so every layout still trains the same model.
            mult = math.lcm(max(1, int(model_cfg.vocab_pad_multiple)), 64 * tp)
            if mult != model_cfg.vocab_pad_multiple:
                model_cfg = replace(model_cfg, vocab_pad_multiple=mult)
                self.mcfg = model_cfg
        # FP8 forward GEMMs (models/gpt.py enable_fp8_forward): what it does not cover is refused here, by name
        if train_cfg.fwd_gemm_dtype not in ("bf16", "fp8", "mxfp8"):
            raise ValueError(f"fwd_gemm_dtype={train_cfg.fwd_gemm_dtype!r}: expected 'bf16', 'fp8' or 'mxfp8'")
        if train_cfg.fwd_gemm_dtype in ("fp8", "mxfp8"):
            why = None
            if train_cfg.dtype == "fp32":
                why = "dtype=fp32 (the exact-fp32 parity mode has no reduced-precision GEMMs)"
            elif tp > 1:
                why = f"tp={tp} (the row-parallel and sequence-parallel forwards are not covered; use tp = 1)"
            elif train_cfg.defer_optimizer:
                why = "defer_optimizer=true (the FP8 weight mirror is rebuilt by the end-of-step update)"
            elif dinfo.device.type == "cuda" and int(os.environ.get("DTC_LN_FUSE", "2")) & 1:
                why = "DTC_LN_FUSE with bit 1 set (the forward LayerNorm fusion runs its own bf16 GEMM)"
            elif model_cfg.d_model % 128 or model_cfg.d_ff % 128:
                why = (f"d_model={model_cfg.d_model}, d_ff={model_cfg.d_ff} (the FP8 GEMM's k-step is 128: both must "
                       "be multiples of 128)")
            if why:
                raise ValueError(f"fwd_gemm_dtype={train_cfg.fwd_gemm_dtype} cannot be combined with {why}")
        rehearse = bool(train_cfg.dp_comm_rehearsal and dp == 1 and dist.is_available() and dist.is_initialized())
        self.mesh: Mesh = build_mesh(dinfo.rank, dinfo.world, dp, tp, pp, dp_group_always=rehearse)
        m = self.mesh
        # the DP code path (bucketed all-reduces, embedding gather, loss all-reduce, ZeRO-1 collectives) runs
        # when there is more than one replica -- or, as a rehearsal, on a one-member DP group
        self.dp_comm = dp > 1 or (rehearse and m.dp_group is not None)
        on_gpu = self.device.type == "cuda"
        self.act_dtype = torch.bfloat16 if (on_gpu and train_cfg.dtype == "bf16") else torch.float32

        # ---- batch geometry (reference: `batch` is the global batch, train_config_*.yaml:1)
        T = model_cfg.max_seq_len
        self._D = model_cfg.d_model
        self.T = T
        self.global_batch = train_cfg.batch
        if self.global_batch % dp:
            raise ValueError(f"global batch {self.global_batch} not divisible by dp={dp}")
        self.b_local = self.global_batch // dp
        self.n_micro = max(1, train_cfg.pp_microbatches) if pp > 1 else self.grad_accum
        if self.b_local % self.n_micro:
            raise ValueError(f"local batch {self.b_local} not divisible by "
                             f"{'pp_microbatches' if pp > 1 else 'grad_accum'}={self.n_micro}")
        self.mb_rows = self.b_local // self.n_micro
        self.row0 = m.dp_idx * self.b_local

        # ---- ownership
        if train_cfg.pp_schedule not in ("gpipe", "1f1b", "zb"):
            raise ValueError(f"pp_schedule={train_cfg.pp_schedule!r}: expected 'gpipe', '1f1b' or 'zb'")
        if train_cfg.pp_split not in ("cost", "even"):
            raise ValueError(f"pp_split={train_cfg.pp_split!r}: expected 'cost' or 'even'")
        weights = None
        if pp > 1 and train_cfg.pp_split == "cost":
            hc = train_cfg.pp_head_cost
            weights = (0.05, head_cost_blocks(model_cfg) if hc is None else float(hc))
        hstages = 2 if self.pp_head_split else 1
        if hstages == 2 and weights is None:
            weights = (0.0, 0.0)  # even split over the stages before the head halves
        layer_ranges = split_layers(model_cfg.n_layers, pp, weights, head_stages=hstages)
        self.layer_ranges = layer_ranges
        head_stage = m.pp_idx >= pp - hstages
        self.layout = StageLayout(layer_ranges[m.pp_idx], has_embed=m.pp_idx == 0, has_head=head_stage,
                                  head_part=(m.pp_idx - (pp - 2), 2) if hstages == 2 and head_stage else (0, 1))
        specs = stage_param_specs(model_cfg, self.layout.layers, self.layout.has_embed, self.layout.has_head,
                                  head_part=self.layout.head_part)
        self.flat = FlatParams(specs, m.tp_idx, tp, self.device, compute_dtype=self.act_dtype)
        if self.act_dtype == torch.bfloat16 and os.environ.get("DTC_DGRAD_NT", "1") == "1":
            # Dense / lm_head dgrads as NT GEMMs on a transposed bf16 weight copy (buffers.enable_transposed)
            # (fc2's dgrad + dGELU runs NN on the row-major weight: level with the NT form on a mirror,
            # profiles/r5_gemm8r.md, so fc2 needs no transposed copy)
            dense = ["fc1", "qkv", "out"]
            head = ["lm_head.w"] if os.environ.get("DTC_DGRAD_NT_HEAD", "1") == "1" else []
            self.flat.enable_transposed([f"h.{l}.{n}.w" for l in self.layout.layers for n in dense] + head)
        self.flat.init_canonical(train_cfg.seed)

        # ---- step program, comms, model, optimizer
        cap = train_cfg.capture_comms
        if cap is None:
            # auto: captured on a one-rank RCCL group (the rehearsal, where it was measured: -0.23 ms) and
            # wherever DTC_CAPTURE_COMMS=1 asks for it; a multi-rank step cuts its graph at each collective
            # (the eager path) until capture has run against real peers over xGMI -- an RCCL kernel that
            # misbehaves inside a capture costs the whole run, an eager one a fraction of a millisecond
            env = os.environ.get("DTC_CAPTURE_COMMS", "auto")
            cap = dinfo.backend == "nccl" and (env == "1" or (env == "auto" and dinfo.world == 1))
        self.program = StepProgram(self.device, use_graph=train_cfg.use_graph and on_gpu, capture_comms=cap)
        # gloo on GPU tensors (the one-GPU multi-rank rig): collectives complete where they are issued,
        # so no copy-back from gloo's worker thread can queue behind a later cross-process wait
        # (parallel/dist.py explains the ordering argument)
        self.program.sync_comms = bool(on_gpu and dinfo.backend == "gloo" and (dinfo.world > 1 or self.dp_comm))
        # every object with a device error word, in the order of the words loss_handle copies: filled by _register
        # where each is created; close, check_health, _err_words and read_loss go through it
        self._transports = {name: None for name in ("p2p", "pp_pipe", "pp_ar", "dp_p2p", "ln")}
        self.p2p = None
        self.pp_pipe = None  # pp_comm: p2p -- the stage messages (created with the message buffers below)
        self.pp_ar = None    # ... and the PP group's scalar sums (loss, pp_clip: global norm)
        self.dp_p2p = None   # dp_comm: p2p -- buckets, loss sum and embedding gather (created with the buffers below)
        mode = train_cfg.tp_comm
        if tp > 1 and on_gpu and (mode == "p2p" or (mode == "auto" and dinfo.backend == "nccl")):
            from ..parallel.p2p import P2PAllReduce

            rows = self.mb_rows if pp > 1 else self.b_local
            self.p2p = self._register("p2p", P2PAllReduce(m.tp_group, m.tp_idx, tp, self.device,
                                                          rows * T * model_cfg.d_model * 4))
        self.tp_comm = TPComm(m.tp_group, tp, m.tp_idx, self.program, p2p=self.p2p)
        self.stage = GPTStage(model_cfg, self.flat, self.layout, self.tp_comm, dropout_seed=train_cfg.seed,
                              act_dtype=self.act_dtype)
        tcd = train_cfg.tp_comm_dtype
        if tcd not in ("fp32", "bf16", "auto"):
            raise ValueError(f"tp_comm_dtype={tcd!r}: expected 'fp32', 'bf16' or 'auto'")
        if tcd == "auto":
            tcd = "bf16" if self.act_dtype == torch.bfloat16 else "fp32"
        self.tp_comm_dtype = tcd
        self.stage.tp_bf16 = bool(tp > 1 and tcd == "bf16")
        sp = train_cfg.tp_sequence_parallel
        # (under grad_accum every microbatch must split into whole sequences over tp: mb_rows == b_local at k = 1)
        sp_rows = self.mb_rows if pp == 1 else self.b_local
        if sp is None:  # auto: wherever it applies
            sp = tp > 1 and pp == 1 and sp_rows % tp == 0
        if sp:
            if tp == 1:
                if dinfo.rank == 0:
                    warnings.warn("tp_sequence_parallel ignored: tp == 1")
            elif pp > 1:
                raise ValueError("tp_sequence_parallel needs pp == 1 (one stage holds the embedding and the head)")
            elif not self.stage.enable_sequence_parallel(sp_rows):
                raise ValueError(f"tp_sequence_parallel: the local batch {self.b_local} must split into whole "
                                 f"sequences over tp={tp}" + (f" in each of its {self.grad_accum} microbatches "
                                                              f"of {self.mb_rows} rows" if self.grad_accum > 1 else ""))
        # deferred grouped weight gradients (models/gpt.py set_wgrad_group): all layers + the lm_head in
        # one launch when no collective waits on per-layer grads (dp == 1), else groups of wgrad_group
        # layers so each group's DP buckets go out under the next group's backward
        wg = train_cfg.wgrad_group
        if wg is None:
            wg = 0 if not self.dp_comm else 2
            if wg == 0:
                wg = self._wgrad_group_for_memory(model_cfg, len(self.layout.layers))
        if pp > 1 and train_cfg.pp_schedule == "zb" and wg < 0:
            # the zero-bubble schedule runs each microbatch's weight gradients (W) apart from its
            # input-gradient chain (B): that needs the deferred grouped path.  Refused here, before any
            # collective, instead of inside the first backward (where only some ranks would raise)
            raise ValueError("pp_schedule='zb' needs deferred weight gradients: wgrad_group >= 0 (or unset)")
        self.stage.set_wgrad_group(wg)
        # DP embedding-grad gather (pp == 1): instead of all-reducing the dense wte/wpe grads
        # (103 MB fp32 for the reference vocab, issued last -> fully exposed), all-gather the
        # embedding-output grads (b_local*T*D fp32 per rank) and let every rank rebuild the
        # identical wte/wpe grads from the global batch with the deterministic sorted kernel.
        if train_cfg.zero_stage not in (0, 1):
            raise ValueError(f"zero_stage={train_cfg.zero_stage}: only 0 (replicated Adam state) and 1 (ZeRO-1) "
                             "are implemented")
        self.zero = bool(train_cfg.zero_stage == 1 and self.dp_comm)
        if self.zero and (tp > 1 or pp > 1):
            raise ValueError("zero_stage=1 is implemented for pure data parallelism (tp = pp = 1)")
        if train_cfg.zero_stage == 1 and not self.dp_comm and dinfo.rank == 0:
            warnings.warn("zero_stage=1 ignored: dp == 1 (nothing to shard); running the replicated AdamW")
        if self.zero and train_cfg.defer_optimizer and dinfo.rank == 0:
            warnings.warn("defer_optimizer ignored under zero_stage=1 (the sharded update ends the step)")
        # zero_comm: p2p -- the sharded step on the in-graph transport (only with self.zero: checked at the top)
        self.zero_p2p = bool(self.zero and train_cfg.zero_comm == "p2p")
        if self.zero and not self.zero_p2p and train_cfg.dp_grad_dtype == "bf16" and dinfo.rank == 0:
            warnings.warn("dp_grad_dtype=bf16 ignored under zero_stage=1: ShardedAdamW reduce-scatters the fp32 grads")
        if self.stage.tp_bf16 and self.stage.wg_group < 0 and dinfo.rank == 0:
            warnings.warn("tp_comm_dtype=bf16 with wgrad_group=-1: the row-parallel "
                          "partials travel as bf16, the input-gradient partials stay fp32")
        self.embed_gather = bool(self.dp_comm and pp == 1 and train_cfg.dp_embed_gather and self.layout.has_embed
                                 and not self.zero and not self.stage.sp)
        bnd = None
        if pp == 1 and len(self.layout.layers):
            names = list(self.flat.slots)
            ends = [self.flat.range_of([n for n in names if n.startswith(f"h.{l}.")])[1] for l in self.layout.layers]
            head = [n for n in names if n.startswith("lm_head") or n.startswith("lnf")]
            bnd = ends + ([self.flat.range_of(head)[1]] if head else [])
        self.buckets = GradBuckets(self.flat, m.dp_group, dp, self.program, train_cfg.dp_bucket_mb,
                                   tail_mb=train_cfg.dp_tail_mb,
                                   local_names=("wte", "wpe") if self.embed_gather else (), boundaries=bnd,
                                   payload=train_cfg.dp_grad_dtype, active=self.dp_comm,
                                   transport="p2p" if self.zero_p2p else train_cfg.dp_comm)
        if self.zero_p2p:
            self.opt = P2PShardedAdamW(self.flat, opt_cfg, self.program, self.buckets.buckets, dp, m.dp_idx,
                                       train_cfg.dp_grad_dtype)
        elif self.zero:
            self.opt = ShardedAdamW(self.flat, opt_cfg, self.program, m.dp_group, dp, m.dp_idx)
        else:
            self.opt = FusedAdamW(self.flat, opt_cfg, self.program, tp, m.tp_group, m.pp_group,
                                  pp_global_clip=(train_cfg.pp_clip == "global"))
        self.opt.reducer = self.stage.red
        if not self.zero:
            self.opt.tp_comm = self.tp_comm
        if pp == 1 and not self.zero:
            # incremental Σg²: with dp == 1 each layer's grads are final when its backward ends
            # (norm chunk per layer, in the layer's batched reduction launch); with dp > 1 only the locally
            # built embedding grads are final before the all-reduces finish
            if not self.dp_comm:
                bk = self.buckets
                cuts = [bk.head_end_offset()] + [bk.layer_end_offset(l) for l in reversed(self.layout.layers)]
                self.opt.set_chunks(sorted(set(c for c in cuts if 0 < c < self.flat.numel)) + [self.flat.numel])
                # the grouped weight-gradient launch also emits its tiles' Σ dW² (the final grads at
                # dp == 1), so the norm pass skips ~3/4 of the grads (DTC_FUSED_NORM=0: off)
                self.stage.wg_record = (on_gpu and self.stage.wg_group == 0 and self.act_dtype == torch.bfloat16
                                        and os.environ.get("DTC_FUSED_NORM", "1") == "1")
            elif self.embed_gather:
                self.opt.set_chunks([self.buckets.reduce_end, self.flat.numel])
        if on_gpu and pp == 1 and self._emb_fused_norm():
            # one local embedding backward per step writes the wte grad: zero only the rows the previous step
            # wrote instead of the 154 MB table (GPT-2 small)
            self.stage.emb_prev = torch.zeros(self.b_local * self.T, dtype=torch.int32, device=self.device)

        # ---- static device-side inputs/outputs (graph replay reads/writes these)
        D = model_cfg.d_model
        if self.embed_gather:
            self.ids_all = torch.zeros(self.global_batch, T, dtype=torch.int32, device=self.device)
            self.ids = self.ids_all[self.row0:self.row0 + self.b_local]  # contiguous row view
            self.dh_all = torch.zeros(self.global_batch * T, D, dtype=torch.float32, device=self.device)
            # dp_grad_dtype: bf16 -> the gather moves the bf16 copy the LayerNorm backward already wrote (half the
            # bytes: 100 MB instead of 201 MB per step at dp8, GPT-2 small), widened once before the backward
            self.dh_all_bf = (torch.zeros(self.global_batch * T, D, dtype=torch.bfloat16, device=self.device)
                              if train_cfg.dp_grad_dtype == "bf16" and self.act_dtype == torch.bfloat16 else None)
            self.feed_row0, self.feed_rows = 0, self.global_batch
        else:
            self.ids = torch.zeros(self.b_local, T, dtype=torch.int32, device=self.device)
            self.feed_row0, self.feed_rows = self.row0, self.b_local
        self.labels = torch.zeros(self.b_local, T, dtype=torch.int32, device=self.device)
        pin = on_gpu
        self._host = [torch.zeros(2, self.feed_rows, T, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._host_i = 0
        self._staged_slot = None  # pinned slot holding the batch stage_batch prepared, until upload_batch
        # the embedding backward's sort keys of the fed ids, sorted on the host while the GPU runs the
        # previous step (a one-block device sort would sit serially in the step: ~48 us)
        self.host_keys = bool(on_gpu and pp == 1 and self.feed_rows * T <= E.SORT_MAX)
        if self.host_keys:
            self._host_keys = [torch.zeros(self.feed_rows * T, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
            self.keys = torch.zeros(self.feed_rows * T, dtype=torch.int32, device=self.device)
        # one host->device copy per step instead of three (ids, labels and sort keys packed in one
        # pinned buffer: each copy is a ~5 us serial node at the head of the step)
        self._packed_in = bool(self.host_keys and not self.embed_gather)
        if self._packed_in:
            self._dev_in = torch.zeros(3, self.feed_rows, T, dtype=torch.int32, device=self.device)
            self.ids, self.labels, self.keys = self._dev_in[0], self._dev_in[1], self._dev_in[2].view(-1)
            self._host = [torch.zeros(3, self.feed_rows, T, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self.grad_accum > 1:
            # every microbatch's embedding-output gradient lands in its rows here; ONE embedding backward per step
            # then runs over the whole local batch (beta 0, the host-sorted keys of the whole batch), so its fused
            # grad-norm partials and sparse zeroing keep their one-writer invariant.  Under the DP embedding gather
            # this is the gather's source (with its bf16 twin where the payload is bf16)
            self.dh_acc = torch.zeros(self.b_local * T, D, dtype=torch.float32, device=self.device)
            self.dh_acc_bf = (torch.zeros(self.b_local * T, D, dtype=torch.bfloat16, device=self.device)
                              if self.embed_gather and self.dh_all_bf is not None else None)
        if train_cfg.dp_comm == "p2p":
            self._init_dp_p2p()
        elif self.zero_p2p:
            self._init_zero_p2p()
        if pp > 1:
            self.recv_x = [torch.zeros(self.mb_rows * T, D, dtype=torch.float32, device=self.device)
                           for _ in range(self.n_micro)]
            self.recv_dx = [torch.zeros(self.mb_rows * T, D, dtype=torch.float32, device=self.device)
                            for _ in range(self.n_micro)]
            self.recv_dx_c = [torch.zeros(self.mb_rows * T, D, dtype=self.act_dtype, device=self.device)
                              for _ in range(self.n_micro)] if self.act_dtype != torch.float32 else self.recv_dx
            # pp_comm_dtype=bf16: stage messages travel as bf16 (send images cast after the producing compute,
            # received images cast back to the fp32 residual stream before the consuming compute)
            pcd = train_cfg.pp_comm_dtype
            if pcd not in ("fp32", "bf16", "auto"):
                raise ValueError(f"pp_comm_dtype={pcd!r}: expected 'fp32', 'bf16' or 'auto'")
            self.pp_bf16 = pcd == "bf16" or (pcd == "auto" and self.act_dtype == torch.bfloat16)
            if self.pp_head_split and m.pp_idx >= pp - 2:
                # the final LayerNorm output (A -> B, compute dtype) and the halves' packed row statistics
                self.recv_yf = [torch.zeros(self.mb_rows * T, D, dtype=self.act_dtype, device=self.device)
                                for _ in range(self.n_micro)]
                self.recv_s = [torch.zeros(self.mb_rows * T, 3, dtype=torch.float32, device=self.device)
                               for _ in range(self.n_micro)]
            if self.pp_bf16:
                mk = lambda: [torch.zeros(self.mb_rows * T, D, dtype=torch.bfloat16, device=self.device)
                              for _ in range(self.n_micro)]
                self.send_x_bf, self.send_dx_bf, self.recv_x_bf, self.recv_dx_bf = mk(), mk(), mk(), mk()
            if train_cfg.pp_comm == "p2p":
                self._init_pp_p2p(pp)
        self.steps_done = 0
        # the evaluation program and its static buffers (evaluate): created by the first evaluation, so a run
        # without one allocates and launches nothing for it
        self.eval_program: Optional[StepProgram] = None
        self.evals_done = 0
        # Deferred optimizer (pp == 1, GPU): the step ends with the global norm and the AdamW of
        # the embedding tables only; the rest of the update runs at the START of the next step
        # on a second stream, in forward order and in a few layer groups, each group signalling
        # an event the forward waits on before its first layer.  The HBM-bound AdamW (~2.2 GB of
        # traffic) then overlaps the compute-bound forward instead of idling the MFMAs at the
        # end of the step.  Semantics are unchanged (same norm, same update, before each use);
        # :meth:`flush_optimizer` completes a pending update (checkpoint, end of run, bench).
        self.defer_opt = bool(on_gpu and pp == 1 and not self.zero and train_cfg.defer_optimizer)
        if self.defer_opt:
            # its own stream: the capped-grid AdamW passes share the CUs with the forward GEMMs instead of
            # queueing ahead of them
            self.opt_stream = torch.cuda.Stream(self.device)
            self._defer_blocks = int(os.environ.get("DTC_DEFER_BLOCKS", "256"))
            self.program.before_comm.append(self._join_opt)
            # device-side "an update is pending" switch: the graph always contains the deferred
            # launch, the kernels skip when nothing is pending (first step, after a flush)
            self._pending_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
            L = list(self.layout.layers)
            bk = self.buckets
            lo_emb = self.flat.range_of([n for n in ("wte", "wpe") if n in self.flat.slots])[0] \
                if self.layout.has_embed else self.flat.numel
            self._emb_range = (lo_emb, self.flat.numel)
            ng = max(1, min(train_cfg.defer_groups, len(L)))
            per = (len(L) + ng - 1) // ng
            self._opt_groups = []  # (first layer, [(lo, hi), ...]) in forward order
            for gi in range(0, len(L), per):
                ls = L[gi:gi + per]
                lo = min(self.flat.range_of([n for n in self.flat.slots if n.startswith(f"h.{l}.")])[0] for l in ls)
                hi = max(bk.layer_end_offset(l) for l in ls)
                self._opt_groups.append((ls[0], [(lo, hi)]))
            if self.layout.has_head:
                self._opt_groups.append(("head", [(0, bk.head_end_offset())]))
        # LayerNorms fused into the layer GEMMs (ops/ln_fused.py).  DTC_LN_FUSE bits: 1 forward
        # (out_proj / fc2 emit the next LayerNorm's output), 2 backward (the fc1 / qkv NT dgrads finish
        # the LayerNorm backward).  Needs tp = pp = 1 (no all-reduce between GEMM and LayerNorm, one call
        # per site and step), a single stream (the row-statistics exchange wants the whole chip for the
        # launch) and, for the backward, the transposed weight mirror.
        lnf = int(os.environ.get("DTC_LN_FUSE", "2"))
        # dp == 1 too: under DP the bucket all-reduces (RCCL kernels on other CUs) run during the
        # backward, and the in-launch row-statistics exchange needs all of its blocks co-resident.
        # grad_accum == 1 too: a fused site is called once per step (its row-statistics epoch is the step counter)
        if (lnf and on_gpu and self.act_dtype == torch.bfloat16 and tp == 1 and pp == 1 and not self.dp_comm
                and not self.defer_opt and self.grad_accum == 1):
            has_wt = len(self.layout.layers) > 0 and self.flat.wt(f"h.{self.layout.layers[0]}.fc1.w") is not None
            if self.stage.enable_ln_fusion(self.b_local * T, self.opt.step_t, fwd=bool(lnf & 1),
                                           bwd=bool(lnf & 2) and has_wt):
                self._register("ln", self.stage.ln_sync)
        if train_cfg.fwd_gemm_dtype == "fp8":
            self.stage.enable_fp8_forward()
        elif train_cfg.fwd_gemm_dtype == "mxfp8":
            self.stage.enable_mxfp8_forward()
        if on_gpu:
            self._reserve_workspaces()

    # ------------------------------------------------------------------ helpers
    def _init_pp_p2p(self, pp: int):
        """``pp_comm: p2p``: the stage messages as in-graph kernels (:class:`parallel.p2p.P2PPipe`; the ``recv_*``
        buffers stay the receive destinations, so every replay moves the same addresses) and a small
        :class:`parallel.p2p.P2PAllReduce` on the PP group for the loss sum and the ``pp_clip: global`` norm
        (scalars padded to 4 floats by :class:`parallel.tp.TPComm`; a rank-order fp32 sum, identical on
        every stage).  With dp == 1 a stage's step then holds no process-group collective at all."""
        from ..parallel.p2p import P2PAllReduce, P2PPipe
        from ..parallel.pp import check_slot_reuse, pp_program, zb_programs

        # the programs this run will execute (zb: placed with this model's costs) must order every slot rewrite
        # after the neighbour's read; deterministic, so every rank raises alike
        kind, hs = self.tcfg.pp_schedule, self.pp_head_split
        progs = (zb_programs(pp, self.n_micro, self.pp_item_costs(), self.pp_comm_costs(), head_split=hs)
                 if kind == "zb" else [pp_program(kind, pp, s, self.n_micro, head_split=hs) for s in range(pp)])
        check_slot_reuse(kind, pp, self.n_micro, hs, progs=progs)
        m, n = self.mesh, self.mb_rows * self.T * self._D
        mdt = torch.bfloat16 if self.pp_bf16 else torch.float32
        msgs = {"f": (n, mdt), "b": (n, mdt)}
        if self.pp_head_split:
            msgs["fh"] = (n, self.act_dtype)
            msgs["s"] = (self.mb_rows * self.T * 3, torch.float32)
        self.pp_pipe = self._register("pp_pipe", P2PPipe(m.pp_group, m.pp_idx, pp, self.device, self.n_micro,
                                                         self.pp_head_split, msgs))
        self.pp_ar = self._register("pp_ar", P2PAllReduce(m.pp_group, m.pp_idx, pp, self.device, 4096,
                                                          label="P2P all-reduce (PP group)", unit="stage"))
        self.pp_sum = TPComm(m.pp_group, pp, m.pp_idx, self.program, p2p=self.pp_ar)
        self.opt.pp_comm = self.pp_sum

    def _init_dp_p2p(self):
        """``dp_comm: p2p``: one :class:`parallel.p2p.P2PGradReduce` on the DP group, sized for the largest
        bucket's payload and for the embedding-gradient gather; the loss becomes the first of 4 floats (the sum
        kernel moves 16-byte pieces, the other three stay zero).  Every call of the step runs on its comm stream;
        the hook re-joins it before a capture ends."""
        from ..parallel.p2p import P2PGradReduce

        m = self.mesh
        gather = 0
        if self.embed_gather:
            gather = (self.dh_all_bf if self.dh_all_bf is not None else self.dh_all).numel() * \
                (2 if self.dh_all_bf is not None else 4)
        self._attach_dp_p2p(P2PGradReduce(m.dp_group, m.dp_idx, m.dp, self.device, self.buckets.buckets,
                                          self.buckets.payload, gather))

    def _init_zero_p2p(self):
        """``zero_comm: p2p``: one :class:`parallel.p2p.P2PZeroShard` on the DP group, sized for the larger of a
        bucket's gradient payload and a rank's fp32 parameter slice of it.  It takes the place of the ``dp_comm:
        p2p`` peer object (``self.dp_p2p``): the loss sum, the comm stream, the join hook, the health check and
        :meth:`close` are the same; the buckets issue reduce-scatters into the optimizer's partial slots."""
        from ..parallel.p2p import P2PZeroShard

        m = self.mesh
        peer = P2PZeroShard(m.dp_group, m.dp_idx, m.dp, self.device, self.buckets.buckets, self.buckets.payload)
        self.opt.attach(peer)
        self.buckets.scatter_parts = self.opt.parts
        self._attach_dp_p2p(peer)

    def _attach_dp_p2p(self, peer):
        """What ``dp_comm: p2p`` and ``zero_comm: p2p`` do alike with their peer object: it carries the buckets, the
        loss becomes the first of the 4 floats its sum kernel moves, and the join hook ends every capture."""
        self.dp_p2p = self._register("dp_p2p", peer)
        self.buckets.peer = peer
        self._loss4 = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.loss = self._loss4[:1]
        self._gather_ev = None
        self.program.before_comm.append(self._join_dp_p2p)

    def _register(self, name: str, transport):
        self._transports[name] = transport
        return transport

    def _live_transports(self):
        return [(name, t) for name, t in self._transports.items() if t is not None]

    def _join_dp_p2p(self):
        if self.dp_p2p is not None:
            self.dp_p2p.join()

    def close(self):
        """Release the peer-to-peer transports (IPC mappings and their uncached buffers)."""
        for name, t in self._live_transports():
            if name != "ln":  # (the fused LayerNorms' granule buffer is an ordinary tensor)
                t.close()
                self._transports[name] = None
                setattr(self, name, None)

    def _wgrad_group_for_memory(self, mc: ModelConfig, n_layers: int) -> int:
        """Auto ``wgrad_group`` at dp == 1: one grouped launch for the whole stage (0) keeps every layer's
        weight-gradient operands alive until the end of the backward -- per layer the bf16 dY tensors
        (dx3, du, dx2, dqkv) and the X operands that would otherwise be freed after its backward (y1, o,
        y2, gelu(u)), (8·D + 2·F)·tokens·2 bytes (GPT-2 small at 8k tokens: 201 MB/layer, 2.4 GB in all).
        When the whole stage's share exceeds the budget (``DTC_WGRAD_MEM_MB``, default 10 % of the
        device's memory, 1 GiB on CPU) the groups shrink to what fits (at least one layer)."""
        if n_layers == 0:
            return 0
        tokens = (self.mb_rows if self.grad_accum > 1 else self.b_local) * self.T  # alive at once
        esize = 2 if self.act_dtype == torch.bfloat16 else 4
        D, F = mc.d_model, mc.d_ff
        per_layer = (8 * D + 2 * F) * tokens * esize
        env = os.environ.get("DTC_WGRAD_MEM_MB")
        if env is not None:
            budget = float(env) * (1 << 20)
        elif self.device.type == "cuda":
            budget = 0.10 * torch.cuda.get_device_properties(self.device).total_memory
        else:
            budget = float(1 << 30)
        if per_layer * n_layers <= budget:
            return 0
        return max(1, int(budget // per_layer))

    def pp_item_costs(self):
        """Per-stage F / B / W costs of one microbatch for the zero-bubble placement (``parallel/pp.py``):
        the stage sizes of the layer split (layers + the head's block-equivalents, ``mesh.stage_costs``).
        Identical on every rank (the programs of all stages must agree)."""
        from ..parallel.mesh import stage_costs
        from ..parallel.pp import stage_item_costs

        hc = self.tcfg.pp_head_cost
        w = (0.05, head_cost_blocks(self.mcfg) if hc is None else float(hc))
        hs = 2 if self.pp_head_split else 1
        return stage_item_costs(self.mesh.pp, stage_costs(self.layer_ranges, w, head_stages=hs),
                                head_half=w[1] / 2 if hs == 2 else 0.0)

    def pp_comm_costs(self):
        """Transfer time of the stage messages in the units of :meth:`pp_item_costs` (one block's F + B + W
        for one microbatch), for the zero-bubble placement: bytes over one xGMI link (assumed 50 GB/s per
        direction) against the block's FLOPs at an assumed 600 TF/s (GPT-2 small: 63 us vs 80 us per
        one-sequence microbatch -- the messages are NOT negligible).  Deterministic, identical on every rank."""
        mc, T, rows = self.mcfg, self.T, self.mb_rows
        D, F = mc.d_model, mc.d_ff
        block_s = 6.0 * (4 * D * D + 2 * D * F + T * D) * rows * T / 600e12
        esz = 2 if getattr(self, "pp_bf16", False) else 4
        fb = rows * T * D * esz / 50e9 / block_s
        return {"f": fb, "b": fb, "s": 1e-5 / block_s}

    def _reserve_workspaces(self):
        from ..ops.gemm import reserve_workspace

        # split-K slabs: the lm_head dgrad (fused CE, split 8 at the reference size) needs 67 MB
        reserve_workspace(self.device, 96 << 20)
        if self.stage.red is not None:
            self.stage.red.reserve()  # the batched-reduction arena: fixed size, held for the engine's lifetime

    @property
    def tokens_per_step(self) -> int:
        return self.global_batch * self.T

    def set_batch(self, batch_np: np.ndarray):
        """batch_np int32 [feed_rows, T+1] (global rows [feed_row0, feed_row0+feed_rows): this rank's
        rows, or the whole global batch under the DP embedding gather) → static device ids/labels."""
        self.stage_batch(batch_np)
        self.upload_batch()

    def stage_batch(self, batch_np: np.ndarray):
        """The host half of :meth:`set_batch`: the token ids / labels into the next pinned host slot and the
        embedding backward's sort keys computed on the host.  A caller that blocks on every step's loss (the
        reference's timed loop, ``bench.py``) stages step t+1's batch while step t still runs on the GPU, so
        only :meth:`upload_batch` (the H2D enqueue) sits between the loss read and the next launch."""
        assert batch_np.shape[0] == self.feed_rows, (batch_np.shape, self.feed_rows)
        i = self._host_i
        h = self._host[i]
        if self._packed_in:
            h[0].copy_(torch.from_numpy(batch_np[:, :-1]))
            h[1].copy_(torch.from_numpy(batch_np[:, 1:]))
            E.embed_sort_keys_host(batch_np[:, :-1], out=h[2].view(-1).numpy())
        else:
            if self.host_keys:
                E.embed_sort_keys_host(batch_np[:, :-1], out=self._host_keys[i].numpy())
            h[0].copy_(torch.from_numpy(batch_np[:, :-1]))
            h[1].copy_(torch.from_numpy(batch_np[:, 1:]))
        self._staged_slot = i
        self._host_i ^= 1

    def upload_batch(self):
        """Enqueue the H2D copies of the batch :meth:`stage_batch` prepared (a two-slot pinned ring: the slot
        is rewritten two batches later, after a loss read has ordered its copy)."""
        i = self._staged_slot
        assert i is not None, "upload_batch without stage_batch"
        self._staged_slot = None
        h = self._host[i]
        if self._packed_in:
            self._dev_in.copy_(h, non_blocking=True)
            return
        if self.host_keys:
            self.keys.copy_(self._host_keys[i], non_blocking=True)
        if self.embed_gather:
            lo = self.row0 - self.feed_row0
            self.ids_all.copy_(h[0], non_blocking=True)
            self.labels.copy_(h[1][lo:lo + self.b_local], non_blocking=True)
        else:
            self.ids.copy_(h[0], non_blocking=True)
            self.labels.copy_(h[1], non_blocking=True)

    # ------------------------------------------------------------------ step bodies
    def _launch_deferred_update(self):
        """Queue the pending AdamW (all but the embedding tables) on the optimizer stream, group by
        group in forward order; each group's event gates the first forward use of its params."""
        if not self.defer_opt:
            return
        st, flag, s = self.stage, self._pending_dev, self.opt_stream
        s.wait_stream(torch.cuda.current_stream())
        for key, ranges in self._opt_groups:
            with torch.cuda.stream(s):
                for lo, hi in ranges:
                    self.opt.update_range(lo, hi, enable=flag, max_blocks=self._defer_blocks)
                ev = torch.cuda.Event()
                ev.record(s)
            st.param_ready[key] = ev

    def _join_opt(self):
        if self.defer_opt:
            torch.cuda.current_stream().wait_stream(self.opt_stream)

    def _finish_optimizer(self):
        if self.defer_opt:
            self.opt.norm()
            self.opt.update_range(*self._emb_range)
            O.fill_(self._pending_dev, 1.0)
        else:
            self.opt.step()

    def flush_optimizer(self):
        """Complete a deferred update now (before reading/saving params or ending a run); the
        next step's in-graph launch then finds nothing pending."""
        if self.defer_opt:
            for _, ranges in self._opt_groups:
                for lo, hi in ranges:
                    self.opt.update_range(lo, hi, enable=self._pending_dev)
            O.fill_(self._pending_dev, 0.0)
            self.stage.param_ready.clear()

    class _CommSafeGemms:
        """GEMM plans for code that runs UNDER asynchronous RCCL collectives (the DP bucket all-reduces
        during the backward, PP send/recv).  RCCL's kernels hold CUs (and LDS) for the whole transfer;
        a GEMM built as exactly one round of one-block-per-CU tiles with all 160 KB of LDS (gemm8n) or
        one ~256-block round of 128 KB-LDS blocks (split-K 256^2 weight gradients) cannot place its last
        blocks until the collective's CUs free up, and would run about twice as long.  Inside this
        context those problems take the many-block 128^2 / 256^2 plans that rebalance over the CUs left (the
        gemm8r plans already have more blocks than CUs and stay).
        No-op on CPU, with a single rank, or with DTC_COMM_SAFE_GEMMS=0."""

        def __init__(self, on: bool):
            self.on = on and torch.cuda.is_available() and os.environ.get("DTC_COMM_SAFE_GEMMS", "1") == "1"

        def __enter__(self):
            if self.on:
                from ..ops import _native as N

                L = N.lib()
                # gemm8r stays (DTC_COMM_SAFE_R8, default 1): 1.5 rounds of two interleaved tile widths, more
                # blocks than CUs, so a CU held by RCCL only delays the blocks it would have run.  One-rank
                # rehearsal with 32 CUs held by a probe kernel: 12.61-12.67 ms/step kept vs 12.77 (and one 20.7
                # outlier) off; with none held 10.97-11.02 vs 11.15-11.20 (profiles/r6_comm_safe_r8.md)
                keep_r8 = os.environ.get("DTC_COMM_SAFE_R8", "1") == "1"
                r8 = L.dtc_gemm_set_r8(0)
                if keep_r8:
                    L.dtc_gemm_set_r8(r8)
                self.prev = (L.dtc_gemm_set_n8(0), L.dtc_gemm_set_wgrad256(0), r8)

        def __exit__(self, *a):
            if self.on:
                from ..ops import _native as N

                L = N.lib()
                L.dtc_gemm_set_n8(self.prev[0])
                L.dtc_gemm_set_wgrad256(self.prev[1])
                L.dtc_gemm_set_r8(self.prev[2])

    def _step_fn_accum(self):
        """``grad_accum: k`` -- the step of :meth:`_step_fn_dp_tp` with the local batch as k microbatches.  Microstep j
        runs rows [j·mb, (j+1)·mb) of the static inputs: the embedding forward with the global row offset of its
        first row (the dropout mask of the unaccumulated step), the head with the full-batch loss scale
        (accumulated into the loss from j = 1 on), the backward with the full-batch gradient scale and beta = 0
        for j = 0, 1 after.  Its saved activations die with its ``ctx`` before the next forward.  Whatever means
        "this gradient is final" -- bucket hooks, norm chunks, the embedding backward, the loss sum, the update --
        belongs to the last microstep (:meth:`_backward_dp_tp` with ``micro``)."""
        st, T, b, k, mb = self.stage, self.T, self.b_local, self.n_micro, self.mb_rows
        dp, dpc, step = self.mesh.dp, self.dp_comm, self.opt.step_t
        hk = self.keys if self.host_keys else None
        out = None
        for j in range(k):
            last = j == k - 1
            ctx: Dict = {}
            r = slice(j * mb, (j + 1) * mb)
            self._doc_bounds_into(ctx, self.ids[r])  # the microstep's own rows
            h = st.embed_forward(self.ids[r], step, self.row0 + j * mb, ctx, want_keys=False)
            h = st.stage_forward(h, mb, ctx)
            st.head_forward(h, self.labels[r], 1.0 / (b * T), ctx, loss_out=self.loss, accumulate=j > 0)
            del h
            gathered = None
            if last:
                if dpc:
                    self._loss_allreduce(name="loss_dp")  # final after the last forward; under the last backward
                if self.embed_gather:
                    gathered = (self.ids_all, 0, (hk, None) if hk is not None else st.embed_keys(self.ids_all))
                else:  # the one embedding backward of the step: the whole local batch
                    full = (hk, None) if hk is not None else st.embed_keys(self.ids)
                    ctx["embed"] = (self.ids, self.row0, full)
                    if st.sp:  # its rows arrive gathered over the TP group already (per microstep, below)
                        gathered = ctx["embed"]
            # only the last backward runs under the bucket collectives
            with self._CommSafeGemms(dpc and last and self.stage.flat.device.type == "cuda"):
                out = self._backward_dp_tp(ctx, dp, step, gathered, micro=(j, k))
            del ctx
        return out

    def _doc_bounds_into(self, ctx: Dict, ids: torch.Tensor):
        """``doc_mask_token`` >= 0: the document bounds of these rows (one launch, inside the step program, from its
        static ids) as ``ctx["doc"]``, where the stage's attention calls look for them.  Off: nothing."""
        if self.doc_token >= 0:
            ctx["doc"] = A.doc_bounds(ids, self.doc_token)

    def _accum_dx(self, j: int, dx: torch.Tensor, dx_c: Optional[torch.Tensor] = None):
        """Microstep j's embedding-output gradient into its rows of the full-batch buffer (``grad_accum``)."""
        n = self.mb_rows * self.T
        if self.stage.sp:
            dx = self.tp_comm.all_gather_rows(dx)  # the microbatch's rows of every TP rank, in row order
        self.dh_acc[j * n:(j + 1) * n].copy_(dx)
        if self.dh_acc_bf is not None and dx_c is not None and dx_c.dtype == torch.bfloat16:
            self.dh_acc_bf[j * n:(j + 1) * n].copy_(dx_c)

    def _step_fn_dp_tp(self):
        if self.grad_accum > 1:
            return self._step_fn_accum()
        st, T, b = self.stage, self.T, self.b_local
        self._launch_deferred_update()
        dp = self.mesh.dp
        dpc = self.dp_comm
        ctx: Dict = {}
        step = self.opt.step_t
        hk = self.keys if self.host_keys else None
        self._doc_bounds_into(ctx, self.ids)
        h = st.embed_forward(self.ids, step, self.row0, ctx, want_keys=not self.embed_gather,
                             keys=None if self.embed_gather else hk)
        gathered = None
        if self.embed_gather:
            gathered = (self.ids_all, 0, (hk, None) if hk is not None else st.embed_keys(self.ids_all))
        h = st.stage_forward(h, b, ctx)
        st.head_forward(h, self.labels, 1.0 / (b * T), ctx, loss_out=self.loss)
        if dpc:
            # the loss is final here: its DP mean goes out now, under the whole backward, instead of
            # as an exposed collective at the end of the step (joined before the optimizer)
            self._loss_allreduce(name="loss_dp")  # (pp == 1 here)
        with self._CommSafeGemms(dpc and self.stage.flat.device.type == "cuda"):  # bucket all-reduces overlap it
            return self._backward_dp_tp(ctx, dp, step, gathered)

    def _backward_dp_tp(self, ctx, dp, step, gathered, micro=None):
        st, T, b = self.stage, self.T, self.b_local
        j, k = micro if micro is not None else (0, 1)  # grad_accum: microstep j of k (the scales stay full-batch)
        beta = 0.0 if j == 0 else 1.0
        if j < k - 1:
            # not the last microstep: the gradients are partial sums.  No bucket, no norm chunk, no TP sum of the
            # sequence-parallel partials (they are summed once, accumulated), no embedding backward, no update
            st.sp_hold = st.sp
            dx, dx_c = st.head_backward(ctx, grad_scale=1.0 / (b * T * dp), beta=beta)
            dx, dx_c = st.stage_backward(ctx, dx, dx_c, beta)
            st.sp_hold = False
            self._accum_dx(j, dx, dx_c)
            return self.loss
        dx, dx_c = st.head_backward(ctx, grad_scale=1.0 / (b * T * dp), beta=beta)
        bk, opt = self.buckets, self.opt
        side = st.red  # grad-norm chunks: into the reducer's batched launches (None: computed right away)
        # deferred weight gradients: the head's grads are final only after the first grouped launch, so
        # what would follow the head backward runs at the first layer hook (which fires after it)
        head_later = [st._defer_wg]
        if not self.dp_comm:
            if not head_later[0]:
                opt.ready_upto(bk.head_end_offset(), side)

            def hook(l):
                if head_later[0]:
                    opt.ready_upto(bk.head_end_offset(), side)
                    head_later[0] = False
                opt.ready_upto(bk.layer_end_offset(l), side)
        else:
            # layer l's grads are final once its reduction launch is queued (before the hook), so its
            # bucket goes out right away; the head's bucket right after the head backward.  The first
            # layer's bucket waits for the embedding gather (that collective feeds compute; the bucket
            # only the optimizer).
            first = self.layout.layers[0]
            per_bucket = not self.zero or self.zero_p2p  # (ZeRO-1 over rccl: ShardedAdamW.step reduce-scatters)
            if per_bucket and not head_later[0]:
                bk.ready_upto(bk.head_end_offset())

            def hook(l):
                if head_later[0]:
                    head_later[0] = False
                    if per_bucket:
                        bk.ready_upto(bk.head_end_offset())
                if self.embed_gather and l == first:
                    return
                bk.ready_upto(bk.layer_end_offset(l))
        if self.zero and not self.zero_p2p:
            hook = None  # grads are reduce-scattered in one call by ShardedAdamW.step
        dx_hook = None
        if self.embed_gather:
            # the embedding-output gradients go out the moment the first layer's dgrad produces them,
            # under that layer's remaining weight-gradient work
            def dx_hook(d, d_c, out=self.dh_all, g=self.mesh.dp_group):
                if k > 1:  # the gather's source is the whole local batch: this microbatch's rows complete it
                    self._accum_dx(j, d, d_c)
                    d, d_c = self.dh_acc, (self.dh_acc_bf if self.dh_acc_bf is not None else self.dh_acc)
                if self.dh_all_bf is not None and d_c.dtype == torch.bfloat16:
                    out, d = self.dh_all_bf, d_c
                ar = self.dp_p2p
                if ar is not None:  # in-graph: on the comm stream, behind the buckets issued so far
                    self._gather_ev = ar.on_comm(lambda: ar.all_gather(d, out), keep=(d,), mark=True)
                    return
                self.program.comm(lambda: dist.all_gather_into_tensor(out, d, group=g),
                                  sig=csig("all_gather", g, d))
        dx, dx_c = st.stage_backward(ctx, dx, dx_c, beta, hook=hook, dx_hook=dx_hook)
        if self.embed_gather:
            bk.ready_all()
            if self.dp_p2p is not None:  # the gather feeds the embedding backward; the buckets behind it do not
                self.dp_p2p.wait_for(self._gather_ev)
                self._gather_ev = None
            if self.dh_all_bf is not None:
                from ..ops.payload import cast_bf16_to_f32

                cast_bf16_to_f32(self.dh_all_bf, self.dh_all)
            st.embed_backward(ctx, self.dh_all, step, 0.0, gathered=gathered)
            opt.chunk_ready(len(opt.chunks) - 1, side)  # local wte/wpe grads: overlaps the tail bucket
        elif k > 1:
            self._accum_dx(j, dx, dx_c)
            st.embed_backward(ctx, self.dh_acc, step, 0.0, gathered=gathered)  # (gathered: sequence parallel only)
        else:
            st.embed_backward(ctx, dx, step, 0.0)
        if self.zero_p2p:
            # every bucket's reduce-scatter and the loss sum joined; P2PShardedAdamW.step pads the step's calls
            # to an even count after its parameter gathers
            if opt.reducer is not None:
                opt.reducer.flush_all()  # grads must be final (launches nothing when every window was flushed)
            bk.ready_all()
            bk.wait_all()
        elif not self.zero:
            bk.ready_all()
            if self.dp_p2p is not None:
                # an even number of calls per step (every replay starts on the same buffer half); a barrier
                # round is a cross-process wait, so it goes to the comm stream like every other call
                self.dp_p2p.on_comm(self.dp_p2p.end_step)
            bk.wait_all()
        if self.dp_comm and self.dp_p2p is None:
            self.program.wait("loss_dp")
        self._finish_optimizer()
        return self.loss

    def _loss_allreduce(self, name: Optional[str] = None, pp: bool = False):
        """Sum the loss over the DP group (and the PP group with ``pp``: only the last stage holds
        it).  With ``name`` the all-reduces are asynchronous: :meth:`StepProgram.wait` joins them
        later (the loss is read by the host only, nothing in the step consumes it)."""
        m = self.mesh
        groups = []
        if self.dp_comm:
            groups.append(m.dp_group)
        if m.pp > 1 and pp:
            groups.append(m.pp_group)
        if not groups:
            return []
        t = self.loss
        if self.dp_p2p is not None:  # dp_comm: p2p (pure DP) -- joined with the buckets, before the optimizer
            ar = self.dp_p2p
            ar.on_comm(lambda: ar.all_reduce_(self._loss4))
            return []
        if self.pp_ar is not None and m.pp > 1 and pp:
            # pp_comm: p2p -- the PP sum is an in-graph kernel (the other stages hold zeros: exact in any order)
            self.pp_sum.all_reduce_(t)
            groups = [g for g in groups if g is not m.pp_group]
            if not groups:
                return []
        if name is None:
            for g in groups:
                self.program.comm(lambda g=g: dist.all_reduce(t, group=g), sig=csig("all_reduce", g, t))
            return []
        # one collective item (one graph cut): with both groups the pp sum must land before the dp
        # sum reads the tensor (separate communicators / streams), so the first is joined to the
        # issuing stream and only the last stays asynchronous
        def fn():
            for g in groups[:-1]:
                dist.all_reduce(t, group=g, async_op=True).wait()
            return dist.all_reduce(t, group=groups[-1], async_op=True)

        self.program.comm(fn, name=name, sig=[x for g in groups for x in csig("all_reduce", g, t)])
        return [name]

    def _step_fn_pp(self):
        from ..parallel.pp import run_pipeline

        # send/recv overlap compute.  Kept under pp_comm: p2p too, where no RCCL kernel holds CUs: dropping it
        # there changes GEMM plans and waits for an A/B on hardware (docs/CAPTURE.md)
        with self._CommSafeGemms(self.stage.flat.device.type == "cuda"):
            run_pipeline(self)
        self.buckets.ready_all()
        # the loss sum overlaps the bucket all-reduces and the optimizer; joined at the very end
        waits = self._loss_allreduce(name="loss_pp", pp=True)
        self.buckets.wait_all()
        self.opt.step()
        for n in waits:
            self.program.wait(n)
        return self.loss

    def _step_fn(self):
        out = self._step_fn_pp() if self.mesh.pp > 1 else self._step_fn_dp_tp()
        if self.p2p is not None:
            self.p2p.end_step()  # even P2P calls per step: every call site keeps its buffer half on replay
        if self.pp_ar is not None:
            self.pp_ar.end_step()
        return out

    # ------------------------------------------------------------------ public
    def run_step(self) -> torch.Tensor:
        """Enqueue one full training step on the static inputs; returns the (device) loss."""
        p = self.program
        p.begin_step()
        check = self.steps_done == 0 or (p.use_graph and not p.recorded)
        if check:
            p.collect()  # the first eager step and the recorded step prove the ranks agree
        if not p.use_graph:
            self._step_fn()
        elif not p.recorded:
            if self.steps_done == 0:
                self._step_fn()  # eager first step: lazy RCCL init, workspace sizing
            else:
                p.record(self._step_fn)
                p.verify("recorded step")
                p.replay()
        else:
            p.replay()
        if check and p.sigs is not None:
            p.verify("first step")
        self.steps_done += 1
        st = self.stage
        if st.wg_record and st.wg_sq is None and st.wg_seen is not None:  # after the first (eager) step
            self.register_fused_norm(st.wg_seen)
        return self.loss

    def register_fused_norm(self, problems):
        """Switch the global norm to the fused Σg² partials: the grouped weight-gradient launch's per-tile Σ dW² over
        ``problems`` (``(dw, n_out, n_in)`` in launch order) and, where it applies, the embedding backward's own.
        :meth:`run_step` calls it with the problems the first, eager step recorded; :meth:`resume_fused_norm` with
        the stage's own list.  ``GPTStage.flush_wgrads`` then refuses a launch over other problems."""
        st = self.stage
        ranges, tiles = [], 0
        base = self.flat.grads.data_ptr()
        for dw, m, n in problems:
            ranges.append(((dw.data_ptr() - base) // 4, dw.numel()))
            tiles += G.wgrad_tiles(m, n)
        nwg = tiles * G.WG_SQ_SLOTS
        # the embedding tables' Σg² from the embedding backward itself (its last kernel writes the final
        # rows): no 154 MB norm pass over a table whose untouched rows are zero (GPT-2 small: -25 us/step)
        emb = 0
        if self._emb_fused_norm():
            for name in ("wte", "wpe"):
                g = self.flat.g(name)
                ranges.append(((g.data_ptr() - base) // 4, g.numel()))
            emb = E.embed_sq_slots(self.b_local, self.T, self._D)
        part = self.opt.set_fused_sumsq(ranges, nwg + emb)
        st.use_wgrad_sumsq(part[:nwg], problems)
        if emb:
            st.emb_sq = part[nwg:]

    def resume_fused_norm(self):
        """After a checkpoint was loaded into an engine that has not stepped yet: register the fused Σg² partials now
        instead of after the first step.  The first step of a resumed process is a later step of the run it
        continues, where the norm comes from the partials (another summation order than the plain pass: a last-bit
        difference in the clip factor flips bf16 mirror roundings); with this it computes what that step computes
        in the uninterrupted run.  A freshly started run is untouched."""
        st = self.stage
        if st.wg_record and st.wg_sq is None and self.steps_done == 0:
            self.register_fused_norm(st.wgrad_problems())

    # ------------------------------------------------------------------ evaluation
    def _eval_fn(self):
        """One evaluation batch on the static evaluation inputs: the training forward with dropout 0 and without
        the GEMM-fused LayerNorm, each layer's saved activations dropped as it returns, the logits-free head.
        ``eval_loss`` = the batch's mean loss over this rank's rows exactly as the training forward computes it
        (the local batch as ``grad_accum`` microbatches with the full-batch scale, accumulated in microbatch
        order), ``eval_count`` = its rows whose arg-max is the label.  Reads the parameters and nothing else of
        the training state: not the step counter's value (dropout 0), not ``emb_prev`` / ``emb_sq`` / the weight-
        gradient records (backward-side), and it ends with its own ``end_step`` so the P2P calls of every program
        stay even (``P2PAllReduce.check``)."""
        st, T, b, k, mb = self.stage, self.T, self.b_local, self.n_micro, self.mb_rows
        self.eval_count.zero_()
        with st.forward_only():
            for j in range(k):
                r = slice(j * mb, (j + 1) * mb)
                ctx: Dict = {}
                self._doc_bounds_into(ctx, self.eval_ids[r])  # evaluation is judged under the mask it trains with
                h = st.embed_forward(self.eval_ids[r], self.opt.step_t, self.row0 + j * mb, ctx, want_keys=False,
                                     dropout=0.0)
                h = st.stage_forward(h, mb, ctx, keep=False)
                st.head_eval(h, self.eval_labels[r], (self.eval_loss, self.eval_count), 1.0 / (b * T),
                             accumulate=j > 0, ctx=ctx)
                del h, ctx
        if self.p2p is not None:
            self.p2p.end_step()
        return self.eval_loss

    def _eval_setup(self, n_batches: int):
        """The evaluation program, its static device inputs / outputs and the held-out batches of this rank's
        rows in pinned host memory (``data/synthetic.py heldout_rows``; built once, re-read by every evaluation)."""
        from ..data import synthetic

        on_gpu = self.device.type == "cuda"
        if self.eval_program is None:
            p = self.program
            self.eval_program = StepProgram(self.device, use_graph=p.use_graph, capture_comms=p.capture_comms)
            self.eval_program.sync_comms = p.sync_comms
            self.eval_program.before_comm = p.before_comm
            self.eval_ids = torch.zeros(self.b_local, self.T, dtype=torch.int32, device=self.device)
            self.eval_labels = torch.zeros(self.b_local, self.T, dtype=torch.int32, device=self.device)
            self.eval_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.eval_count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._eval_host = torch.zeros(0, 2, self.b_local, self.T, dtype=torch.int32)
            self._eval_stream = synthetic.SyntheticTokenStream(
                vocab=min(synthetic.BPE_VOCAB, self.mcfg.vocab_size - 1), seed=self.tcfg.seed)
        have = self._eval_host.shape[0]
        if have < n_batches:
            host = torch.zeros(n_batches, 2, self.b_local, self.T, dtype=torch.int32, pin_memory=on_gpu)
            host[:have].copy_(self._eval_host)
            for i in range(have, n_batches):
                rows = synthetic.heldout_rows(self._eval_stream, i, self.row0, self.b_local, self.global_batch,
                                              self.T + 1)
                host[i, 0].copy_(torch.from_numpy(rows[:, :-1]))
                host[i, 1].copy_(torch.from_numpy(rows[:, 1:]))
            self._eval_host = host
        if len(getattr(self, "_eval_out", ())) < n_batches:
            self._eval_out = [(torch.zeros(1, dtype=torch.float32, pin_memory=on_gpu),
                               torch.zeros(1, dtype=torch.int32, pin_memory=on_gpu)) for _ in range(n_batches)]

    def evaluate(self, n_batches: Optional[int] = None) -> Dict:
        """Forward-only pass over the first ``n_batches`` (default ``eval_batches``) held-out batches of ``batch``
        rows: ``dict(loss, ppl, top1, tokens)`` -- mean loss per token, ``exp(loss)``, the share of tokens whose
        arg-max logit is the label, and the tokens evaluated -- the same on every rank.

        The device accumulates per batch (fp32 loss in a fixed order, integer count), the host across batches
        in float64, the DP group with ONE eager all-reduce of a 3-element float64 vector (loss sum, correct,
        tokens) per evaluation; the TP ranks of a replica hold the same numbers already.  The batches replay the
        evaluation's own captured program (:meth:`_eval_fn`; the first evaluation runs its first batch eagerly
        and records on the second, as :meth:`run_step` does), with its own static inputs: the training loop
        stages the next training batch before it reads the previous loss, so the training buffers are never
        free.  Blocking.  Refused before the first training step (the eager step that sizes workspaces and
        initialises the process groups), under pipeline parallelism and with ``defer_optimizer``."""
        if self.mesh.pp > 1:
            raise ValueError("evaluate(): evaluation under pipeline parallelism is not implemented (pp == 1 only; "
                             "the follow-up: a forward-only pipeline schedule)")
        if self.tcfg.defer_optimizer:
            raise ValueError("evaluate(): not with defer_optimizer=true (the deferred update runs under the next "
                             "step's forward: parameters are not final between steps)")
        if self.tcfg.data != "synthetic":
            raise ValueError(f"evaluate(): the held-out set is defined for data: synthetic, not {self.tcfg.data!r}")
        if self.steps_done == 0:
            raise RuntimeError("evaluate() before the first training step: run one step first (it sizes the "
                               "workspaces and initialises the process groups the evaluation forward reuses)")
        n = int(self.tcfg.eval_batches if n_batches is None else n_batches)
        if n < 1:
            raise ValueError(f"evaluate(): n_batches={n}: expected >= 1")
        self._eval_setup(n)
        p, train_p = self.eval_program, self.tp_comm.program
        self.tp_comm.program = p  # the evaluation's TP collectives cut (or join) ITS graph, not the training step's
        try:
            for i in range(n):
                self.eval_ids.copy_(self._eval_host[i, 0], non_blocking=True)
                self.eval_labels.copy_(self._eval_host[i, 1], non_blocking=True)
                p.begin_step()
                check = self.evals_done == 0 or (p.use_graph and not p.recorded)
                if check:
                    p.collect()
                if not p.use_graph or (not p.recorded and self.evals_done == 0):
                    self._eval_fn()
                elif not p.recorded:
                    p.record(self._eval_fn)
                    p.verify("recorded evaluation batch")
                    p.replay()
                else:
                    p.replay()
                if check and p.sigs is not None:
                    p.verify("first evaluation batch")
                self.evals_done += 1
                lo, co = self._eval_out[i]
                lo.copy_(self.eval_loss, non_blocking=True)
                co.copy_(self.eval_count, non_blocking=True)
        finally:
            self.tp_comm.program = train_p
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        self.check_health()
        rows_tokens = self.b_local * self.T
        # per batch: eval_loss = this rank's mean over its b_local * T tokens -> its loss SUM in float64
        loss_sum = sum(float(lo.item()) for lo, _ in self._eval_out[:n]) * rows_tokens
        correct = sum(int(co.item()) for _, co in self._eval_out[:n])
        vec = torch.tensor([loss_sum, float(correct), float(n * rows_tokens)], dtype=torch.float64)
        if self.dp_comm:
            g = self.mesh.dp_group
            if self.dinfo.backend == "nccl":
                vec = vec.to(self.device)
            dist.all_reduce(vec, group=g)
            vec = vec.cpu()
        tokens = int(vec[2].item())
        loss = float(vec[0].item()) / tokens
        return dict(loss=loss, ppl=math.exp(loss) if loss < 700.0 else float("inf"),
                    top1=float(vec[1].item()) / tokens, tokens=tokens)

    def _emb_fused_norm(self) -> bool:
        """The embedding backward alone writes the wte / wpe grads, once per step, and they are final there: dp 1
        (no all-reduce or gather of them), no TP / sequence parallelism (norm weight 1), one sort window.  Then it
        may write the tables' share of Σg² itself and zero only the wte rows its previous call wrote."""
        return (self.layout.has_embed and not self.dp_comm and self.mesh.tp == 1 and not self.embed_gather
                and not self.stage.sp and self.b_local * self.T <= E.SORT_MAX)

    def loss_value(self) -> float:
        """Blocking read of the global mean loss (reference: float(np.asarray(loss)), train.py:82)."""
        v = float(self.loss.item())
        self.check_health()
        return v / self.mesh.dp

    def check_health(self):
        """Raise if a device-side wait of this rank timed out (P2P all-reduce flags, fused LayerNorm
        row statistics).  Blocking: call outside pipelined loops."""
        for _, t in self._live_transports():
            t.check()

    # -- host pipelining: read step t's loss while step t+1 is already queued --------------
    def _err_words(self):
        """Device error words of this rank's in-launch waits (P2P all-reduce flags, fused LayerNorm
        row statistics): nonzero = a wait timed out and that step computed NaN."""
        return [(name, t.err) for name, t in self._live_transports()]

    def loss_handle(self):
        """Queue a copy of this step's loss (and of the error words) to pinned host memory (2-slot
        ring) + an event.

        With the step replayed from a graph, the host can enqueue step t+1 (its H2D batch copy
        and graph launch) before blocking on step t's loss, so the GPU never idles on the host
        between steps; every step's loss is still read (one step later), and a timed-out device
        wait raises at that read instead of letting NaN losses through silently."""
        if self.device.type != "cuda":
            return self.loss_value()
        words = self._err_words()
        if not hasattr(self, "_loss_host"):
            self._loss_host = [torch.zeros(1, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            self._err_host = [torch.zeros(max(1, len(words)), dtype=torch.int32, pin_memory=True) for _ in range(2)]
            self._loss_slot = 0
        i = self._loss_slot
        slot, eslot = self._loss_host[i], self._err_host[i]
        self._loss_slot ^= 1
        slot.copy_(self.loss, non_blocking=True)
        for j, (_, w) in enumerate(words):
            eslot[j:j + 1].copy_(w, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return slot, ev, eslot

    def read_loss(self, handle) -> float:
        if not isinstance(handle, tuple):
            return handle
        slot, ev, eslot = handle
        ev.synchronize()
        for j, (_, t) in enumerate(self._live_transports()):
            e = int(eslot[j])
            if e:
                raise RuntimeError(t.describe(e))
        return float(slot.item()) / self.mesh.dp

    def grad_norm(self) -> float:
        return self.opt.grad_norm()
