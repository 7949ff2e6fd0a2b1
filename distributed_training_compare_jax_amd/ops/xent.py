"""Fused lm_head + softmax cross-entropy (reference ``model/GPTModel.py:71-72`` and
``train/create_train_step.py:32-34``: ``softmax_cross_entropy_with_integer_labels(...).mean()``).

Forward (GPU): ONE MFMA GEMM ``logits = h·Wᵀ + b`` whose epilogue also emits, per row and
per 128-column tile, the partial ``(max, Σexp)`` of the fp32 accumulators and captures the
label logit — the 4096×50304 fp32 logits (823 MB in the reference) are never re-read for
the forward loss.  Logits are kept only as bf16 (412 MB, trivially resident in 288 GB
HBM) for the backward, which is one streaming pass ``dlogits = (softmax − onehot)·scale``
written in place, followed by the two GEMMs of the Dense backward.

The vocab is padded (``ModelConfig.padded_vocab``); pad columns get ``-inf`` logits, so
their probability and gradient are exactly 0 — identical loss to the unpadded reference.
Vocab-parallel TP: each rank owns columns ``[vocab_start, vocab_start+V_local)``; rows'
``(max, Σexp)`` and label logits are combined across ranks (``parallel/tp.py``).
"""

from __future__ import annotations

import torch

from . import _native as N


def lmhead_logits_partials(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor, labels: torch.Tensor,
                           vocab_start: int, n_valid: int, combine: bool = True):
    """Returns ``(logits [M,Vl], rowstat [M,2] (max,Σexp), label_logit [M])`` for the local vocab shard.

    ``n_valid`` = number of real (non-pad) columns in this shard; ``label_logit`` is 0 for rows
    whose label is outside the shard.  ``combine=False`` returns the GEMM's raw per-tile partials
    ``[P, M, 2]`` instead of ``rowstat`` (a single-shard loss feeds them straight to
    :func:`ce_finalize`: one combine launch instead of two)."""
    M, D = h.shape
    Vl = w.shape[0]
    if N.library_path(h):
        logits = h.float() @ w.float().t() + b.float()
        if n_valid < Vl:
            logits[:, n_valid:] = float("-inf")
        mx = logits.max(-1).values
        se = torch.exp(logits - mx[:, None]).sum(-1)
        loc = labels.long() - vocab_start
        inside = (loc >= 0) & (loc < n_valid)
        lab = torch.where(inside, logits.gather(1, loc.clamp(0, Vl - 1)[:, None])[:, 0], torch.zeros(M, device=h.device))
        rs = torch.stack([mx, se], -1)
        return logits.to(h.dtype), (rs if combine else rs.unsqueeze(0)), lab
    L = N.lib()
    f32 = h.dtype == torch.float32  # exact-fp32 parity mode: fp32 logits (csrc/gemm_f32.hip)
    P = int(L.dtc_lmhead_nparts_f32(M, Vl, D) if f32 else L.dtc_lmhead_nparts(M, Vl, D))
    logits = torch.empty(M, Vl, dtype=h.dtype, device=h.device)
    part = torch.empty(P, M, 2, dtype=torch.float32, device=h.device)  # part-major (coalesced epilogue writes)
    # a single shard (combine=False) holds every row's label: the epilogue writes all of lab
    lab = (torch.zeros if combine else torch.empty)(M, dtype=torch.float32, device=h.device)
    from .gemm import _gemm_native

    _gemm_native(0, M, Vl, D, h, h.stride(0), w, w.stride(0), logits, Vl, epi=N.EPI_LMHEAD, bias=b,
                 labels=labels, vocab_start=vocab_start, n_valid=n_valid, part=part, label_out=lab)
    if not combine:
        return logits, part, lab
    return logits, combine_partials(part), lab


def lmhead_eval_partials(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor, labels: torch.Tensor,
                         vocab_start: int, n_valid: int, single_shard: bool = True):
    """The forward-only (evaluation) lm_head: the row statistics of :func:`lmhead_logits_partials` and the
    arg-max candidates of the local vocab shard, with no logits kept.

    Returns ``(part [P, M, 2], label_logit [M], cand_val [Pa, M], cand_col [Pa, M] int32)``: ``part`` and
    ``label_logit`` are what ``lmhead_logits_partials(..., combine=False)`` returns, bit for bit; candidate
    ``p`` of row ``m`` is the shard-local column ``cand_col[p, m]`` (-1: none) holding the value
    ``cand_val[p, m]``, the lowest valid column among equal maxima.  :func:`ce_eval_finish` picks the row's
    winner.  Values are the logits rounded to the activation dtype, pad columns never candidates.

    bf16 on the GPU: one GEMM launch with the ``EPI_LMHEAD_EVAL`` epilogue -- no logits are stored and
    ``cand_val`` is a view of ``part`` (a part's maximum IS the value at its arg-max).  fp32 on the GPU (the
    exact-fp32 parity mode): the storing head, then a streaming row arg-max over its fp32 logits
    (``Pa = 1``).  CPU: pure torch, ``P = Pa = 1``.  ``single_shard=False`` (one of several vocab shards:
    some labels lie outside it): the fp32 head combines its parts as the training head does there
    (``P = 1``); the bf16 epilogue zeroes ``label_logit`` first either way."""
    M, D = h.shape
    Vl = w.shape[0]
    if N.library_path(h) or h.dtype == torch.float32:
        logits, part, lab = lmhead_logits_partials(h, w, b, labels, vocab_start, n_valid, combine=not single_shard)
        if not single_shard:
            part = part.unsqueeze(0)  # the combined (max, sum exp) as the shard's one part
        if N.library_path(h):
            lg = logits.float()  # (rounded to the activation dtype, pads -inf)
            if n_valid > 0:
                val, col = lg[:, :n_valid].max(-1)  # torch.max: the first index among equal maxima
                col = col.to(torch.int32)
            else:
                val = torch.full((M,), float("-inf"))
                col = torch.full((M,), -1, dtype=torch.int32)
            return part, lab, val[None], col[None]
        val = torch.empty(1, M, dtype=torch.float32, device=h.device)
        col = torch.empty(1, M, dtype=torch.int32, device=h.device)
        N.check(N.lib().dtc_row_argmax_f32(logits.data_ptr(), logits.stride(0), M, n_valid, val.data_ptr(),
                                           col.data_ptr(), N.stream_ptr(h.device)), "dtc_row_argmax_f32")
        return part, lab, val, col
    L = N.lib()
    P = int(L.dtc_lmhead_nparts(M, Vl, D))
    part = torch.empty(P, M, 2, dtype=torch.float32, device=h.device)
    col = torch.empty(P, M, dtype=torch.int32, device=h.device)
    lab = torch.zeros(M, dtype=torch.float32, device=h.device)  # rows whose label is outside the shard stay 0
    from .gemm import _gemm_native

    _gemm_native(0, M, Vl, D, h, h.stride(0), w, w.stride(0), None, Vl, epi=N.EPI_LMHEAD_EVAL, bias=b,
                 labels=labels, vocab_start=vocab_start, n_valid=n_valid, part=part, label_out=lab, part_arg=col)
    return part, lab, part[:, :, 0], col


def combine_partials(part: torch.Tensor) -> torch.Tensor:
    """``part [P, M, 2]`` → ``rowstat [M, 2]`` (max, Σexp) of the shard: what
    ``lmhead_logits_partials(combine=True)`` returns for the same partials."""
    P, M, _ = part.shape
    if not part.is_cuda:  # (the CPU paths produce one part)
        assert P == 1
        return part[0]
    rowstat = torch.empty(M, 2, dtype=torch.float32, device=part.device)
    N.check(N.lib().dtc_ce_combine(part.data_ptr(), M, P, 1, M, None, None, rowstat.data_ptr(), 0.0, None, 0,
                                   N.stream_ptr(part.device)), "dtc_ce_combine")
    return rowstat


def ce_eval_finish(cand_val: torch.Tensor, cand_col: torch.Tensor, col_off: int = 0,
                   labels: torch.Tensor | None = None, count: torch.Tensor | None = None):
    """Per row, the winner of ``P`` arg-max candidates ``(cand_val[p, m], cand_col[p, m])``: the largest value,
    the lowest column among equal values; a negative column is no candidate.  ``cand_col`` is int32, or fp32
    holding integers (candidates gathered with the row statistics of R vocab shards).

    Returns ``(argmax [M] int32 = column + col_off, or -1; value [M]; correct [M] int32 or None)``.  With
    ``labels`` (global ids), ``correct = argmax == label`` and the number of correct rows is ADDED to the
    int32 device counter ``count`` (an integer sum: the same in any order)."""
    P, M = cand_val.shape
    assert cand_col.shape == (P, M) and (labels is None) == (count is None)
    dev = cand_val.device
    if not cand_val.is_cuda:
        cols = cand_col.to(torch.int64)
        v = torch.where(cols >= 0, cand_val.float(), torch.full_like(cand_val, float("-inf"), dtype=torch.float32))
        best = v.max(0).values
        win = (v == best[None]) & (cols >= 0)
        big = torch.iinfo(torch.int64).max
        col = torch.where(win, cols, torch.full_like(cols, big)).min(0).values
        am = torch.where(col == big, torch.full_like(col, -1), col + col_off).to(torch.int32)
        correct = None
        if labels is not None:
            correct = (am == labels.reshape(-1).to(torch.int32)).to(torch.int32)
            count.add_(correct.sum().to(count.dtype))
        return am, best, correct
    am = torch.empty(M, dtype=torch.int32, device=dev)
    val = torch.empty(M, dtype=torch.float32, device=dev)
    correct = torch.empty(M, dtype=torch.int32, device=dev) if labels is not None else None
    assert cand_val.dtype == torch.float32 and cand_col.dtype in (torch.int32, torch.float32)
    assert count is None or (count.dtype == torch.int32 and labels.dtype == torch.int32 and labels.is_contiguous())
    N.check(N.lib().dtc_ce_eval_finish(cand_val.data_ptr(), cand_val.stride(1), cand_val.stride(0), cand_col.data_ptr(),
                                       int(cand_col.dtype == torch.float32), cand_col.stride(1), cand_col.stride(0),
                                       M, P, int(col_off), N.ptr(labels), am.data_ptr(), val.data_ptr(),
                                       N.ptr(correct), N.ptr(count), N.stream_ptr(dev)), "dtc_ce_eval_finish")
    return am, val, correct


def ce_finalize(rowstats: torch.Tensor, label_logit: torch.Tensor, loss_scale: float,
                loss_out: torch.Tensor | None = None, accumulate: bool = False):
    """rowstats [R, M, 2] (R vocab shards) + label_logit [M] → (lse [M], loss).

    ``loss = scale·Σ(lse − label)`` (1-element fp32), written to / accumulated into ``loss_out``."""
    R, M, _ = rowstats.shape
    if loss_out is None:
        loss_out = torch.zeros(1, dtype=torch.float32, device=rowstats.device)
    if not rowstats.is_cuda:
        mx = rowstats[..., 0].max(0).values
        s = (rowstats[..., 1] * torch.exp(rowstats[..., 0] - mx[None])).sum(0)
        lse = mx + torch.log(s)
        loss = (lse - label_logit).sum() * loss_scale
        if accumulate:
            loss_out.add_(loss)
        else:
            loss_out.fill_(float(loss))
        return lse, loss_out
    lse = torch.empty(M, dtype=torch.float32, device=rowstats.device)
    assert rowstats.is_contiguous()
    N.check(N.lib().dtc_ce_combine(rowstats.data_ptr(), M, R, 1, M, label_logit.data_ptr(), lse.data_ptr(), None,
                                   loss_scale, loss_out.data_ptr(), 1 if accumulate else 0,
                                   N.stream_ptr(rowstats.device)), "dtc_ce_combine")
    return lse, loss_out


def ce_backward_inplace(logits: torch.Tensor, lse: torch.Tensor, labels: torch.Tensor, vocab_start: int,
                        n_valid: int, grad_scale: float, colpart: bool = False):
    """logits → dlogits = (exp(logits − lse) − onehot)·grad_scale (pad columns 0), in place.

    ``colpart=True`` also returns fp32 column partial sums of dlogits ``[R, V]`` (R row chunks)
    from the same pass — the lm_head bias gradient is their column sum (``gemm.colsum``)."""
    M, Vl = logits.shape
    if N.library_path(logits):
        p = torch.exp(logits.float() - lse[:, None])
        if n_valid < Vl:
            p[:, n_valid:] = 0.0
        loc = labels.long() - vocab_start
        inside = (loc >= 0) & (loc < n_valid)
        # one-hot subtraction without a data-dependent shape (graph-capturable on the GPU fp32 path)
        rows = torch.arange(M, device=logits.device)
        p.index_put_((rows, loc.clamp(0, Vl - 1)), -inside.to(p.dtype), accumulate=True)
        logits.copy_((p * grad_scale).to(logits.dtype))
        if colpart:
            return logits, (p * grad_scale).sum(0, keepdim=True)
        return logits
    L = N.lib()
    cp = None
    if colpart:
        R = (M + int(L.dtc_ce_colsum_rows()) - 1) // int(L.dtc_ce_colsum_rows())
        cp = torch.empty(R, Vl, dtype=torch.float32, device=logits.device)
    fn = L.dtc_ce_bwd_f32 if logits.dtype == torch.float32 else L.dtc_ce_bwd
    N.check(fn(logits.data_ptr(), logits.stride(0), lse.data_ptr(), labels.data_ptr(), M, Vl, vocab_start,
               n_valid, grad_scale, N.ptr(cp), N.stream_ptr(logits.device)), "dtc_ce_bwd")
    return (logits, cp) if colpart else logits


def ce_dgrad_fused(logits: torch.Tensor, lse: torch.Tensor, labels: torch.Tensor, vocab_start: int, n_valid: int,
                   grad_scale: float, wt: torch.Tensor, want_dlogits: bool = True):
    """The lm_head backward's first half in ONE kernel (``csrc/gemm.hip`` ce_dgrad256_kernel): the
    cross-entropy backward applied to the logits as they are staged into the dgrad GEMM.

    Returns ``(dx, dlogits, colpart)``: dx = dlogits·W (fp32 [M, d], ``wt`` = Wᵀ [d, V] bf16),
    dlogits (bf16 [M, V], bitwise equal to :func:`ce_backward_inplace`'s, for the weight gradient)
    and the column partial sums of dlogits (fp32 [R, V], the bias gradient's input — summed from
    the bf16 dlogits, where :func:`ce_backward_inplace` sums the fp32 values before rounding).
    The logits are left untouched.  GPU bf16 path only."""
    from .gemm import _workspace

    M, Vl = logits.shape
    D = wt.shape[0]
    assert wt.shape[1] == Vl and logits.dtype == torch.bfloat16 and wt.dtype == torch.bfloat16
    assert logits.is_contiguous() and wt.is_contiguous()
    L = N.lib()
    dl = torch.empty_like(logits) if want_dlogits else None
    cp = torch.empty(int(L.dtc_ce_dgrad_colpart_rows(M)), Vl, dtype=torch.float32, device=logits.device) \
        if want_dlogits else None
    dx = torch.empty(M, D, dtype=torch.float32, device=logits.device)
    nbytes = int(L.dtc_ce_dgrad_workspace_bytes(M, D, Vl))
    ws = _workspace(logits.device, nbytes)
    N.check(L.dtc_ce_dgrad(logits.data_ptr(), logits.stride(0), lse.data_ptr(), labels.data_ptr(), vocab_start, n_valid,
                           grad_scale, wt.data_ptr(), wt.stride(0), N.ptr(dl), 0 if dl is None else dl.stride(0),
                           N.ptr(cp),
                           dx.data_ptr(), M, D, Vl, ws.data_ptr(), ws.numel(), N.stream_ptr(logits.device)),
            "dtc_ce_dgrad")
    return dx, dl, cp


