"""vgate compute ops: gfx950 HIP kernels (``vgate._C``) with fp32 torch references.

Dispatch rule: GPU tensors ALWAYS go to the native HIP kernels — if the
extension is missing on a GPU machine the op raises (no silent eager fallback);
CPU tensors use the reference implementations in :mod:`vgate.ops.reference`.

This module is the dispatch layer. Weight packing and :class:`Linear` live in :mod:`.packing`, the
per-device buffers in :mod:`.buffers`, the start-up prefill tuner in :mod:`.tuner`, the extension
loader in :mod:`._native`; their names are re-exported here.
"""
from __future__ import annotations

import math

import torch

from . import reference as ref
from ._native import (EPI_BF16, EPI_F32, EPI_QKV, EPI_SILU, PATH_AUTO, PATH_KX, PATH_MID, PATH_PREFILL,  # noqa: F401
                      PATH_STREAMK, native, native_available)
from .buffers import (_TICKETS, _WS, attn_tickets, fault_word, logprob_partials, qa_sync,  # noqa: F401
                      reserve_awq_scratch, reset_handoffs, sample_workspace, sk_workspace, workspace)
from .packing import (Linear, interleave_gate_up, mxfp4_dequant_ref, pack_awq, pack_awq_sz, pack_fp8,  # noqa: F401
                      pack_mxfp4, pack_mxfp4_scales, pack_weight, row_permutation, unpack_awq, unpack_fp8,
                      unpack_mxfp4, unpack_mxfp4_scales, unpack_weight)
from .tuner import (MEDIUM_DEFAULT, MID_BASE, MID_CANDIDATES, PREFILL_CANDIDATES,  # noqa: F401
                    PREFILL_RING_CANDIDATES, _cold_timer, _plan_bucket, _plan_kw, apply_prefill_plans,
                    load_plan_cache, save_plan_cache, tune_prefill, tune_prefill_cached)

# ---- switches: tests flip them by assignment on this module, and the code below reads them at call time
# decode-only steps: the decode attention rides in the QKV projection's launch (qkv_attn.hip); tests
# turn it off to compare against the two-launch path (the o_proj as a third role measured no faster:
# profiles/r5_qa_oproj_negative.log)
FUSE_QKV_ATTN = True
# every dense decode GEMM (<= 16 rows) on the stream-K kernel: one equal share of the packed weight
# stream per CU (csrc/kernels/gemm_streamk.hip); off by default — the measured per-shape plans
# (Linear.dec_sk, vgate/models/decode_plans.py) pick it where it wins; tests turn it on
STREAMK_DECODE = False
# flash prefill: long causal ranges run as two K halves met through fp32 partials in the GEMM
# workspace (csrc/kernels/attention.hip attn_flash_kernel, two blocks per KV head); tests turn it off
FLASH_SPLIT = True
# AWQ steps of 16 < M <= 64 rows (mixed prefill + decode) run the int4 medium kernel; longer ones
# (M >= AWQ_DEQUANT_MIN_M not taken by it) dequantise to scratch + the bf16 prefill / tile kernels
AWQ_DEQUANT_MIN_M = 32


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _prefill_plan_kw(lin: Linear, M: int) -> dict:
    """C.gemm keywords of the Linear's measured plan for a step of M > 16 rows (empty: the launcher's rule)."""
    if M <= 16 or not lin.prefill_plan:
        return {}
    return _plan_kw(lin.prefill_plan.get(_plan_bucket(lin.prefill_plan, M)), M)


def _gemm_route(lin: Linear, M: int, *, waves: int, splitk: int, path: int, row_idx, ar, norm_out) -> tuple:
    """The kernel family one :func:`linear` call asks for, from the caller's knobs and the Linear's plans:
    ("dequant", plan keywords of the bf16 GEMM) or ("gemm", path, waves, splitk, ntb). Touches no tensor,
    buffer or extension. Explicit ``waves`` / ``splitk`` switch every plan off."""
    planned = waves == 0 and splitk == 0
    if lin.kind == "awq" and planned and row_idx is None:
        if 16 < M <= 64 and path == PATH_AUTO and lin.group == 128 and lin.szp is not None:
            return ("gemm", PATH_MID, 0, 0, 0)  # int4 medium kernel (gemm_awq_mid.hip awq_mid_kernel): no bf16 scratch
        if M >= AWQ_DEQUANT_MIN_M:
            return ("dequant", _prefill_plan_kw(lin, M))
    if lin.kind in ("fp8", "mxfp4"):
        # M <= 16: the fp8 / mxfp4 decode kernel (gemm_fp8.hip / gemm_mxfp4.hip; forced waves / splitk are its own
        # knobs); longer steps: fp8 / mxfp4 -> bf16 scratch + the bf16 kernels on the Linear's prefill plan
        if row_idx is not None or ar is not None or norm_out is not None:
            raise ValueError(f"{lin.kind} Linear: no row_idx, fused all-reduce or norm hand-off")
        if M > 16:
            return ("dequant", _prefill_plan_kw(lin, M) if planned and path == PATH_AUTO else
                    dict(waves=waves, splitk=splitk, path=path))
        if planned:
            waves, splitk, ntb = lin.dec_waves, lin.dec_splitk, lin.dec_ntb
            return ("gemm", PATH_AUTO, waves, splitk, ntb)
        return ("gemm", PATH_AUTO, waves, splitk, 0)
    ntb = 0
    if M <= 16 and planned:
        waves, splitk, ntb = lin.dec_waves, lin.dec_splitk, lin.dec_ntb
        dense = lin.kind == "dense" and row_idx is None and ar is None
        if path == PATH_AUTO and dense:
            path = lin.dec_path
        # stream-K decode kernel (csrc/kernels/gemm_streamk.hip): per-Linear plan, else the module default
        if (dense and path == PATH_AUTO and norm_out is None
                and (lin.dec_sk if lin.dec_sk is not None else STREAMK_DECODE)):
            path = PATH_STREAMK  # (W, blocks per CU, k-steps per register group) of the plan, 0 = the kernel's default
            waves, splitk, ntb = lin.dec_sk if isinstance(lin.dec_sk, tuple) else (0, 0, 0)
    elif M > 16 and planned and path == PATH_AUTO and lin.kind == "dense":  # (AWQ: the dequant route above)
        pk = _prefill_plan_kw(lin, M)
        path, waves, splitk, ntb = pk.get("path", PATH_AUTO), pk.get("waves", 0), pk.get("splitk", 0), pk.get("ntb", 0)
    return ("gemm", path, waves, splitk, ntb)


def _norm_kw(norm, rownorm: bool) -> dict:
    """Fused RMSNorm keywords: the row scale alone when gamma lives in the weights, else gamma too."""
    if norm is None:
        return {}
    if rownorm:
        return dict(rownorm=True, eps=float(norm[1]))
    return dict(norm_w=norm[0], eps=float(norm[1]))


def _qkv_kw(qkv) -> dict:
    if qkv is None:
        return {}
    return dict(positions=qkv["positions"], slots=qkv["slots"], cos_sin=qkv["cos_sin"],
                k_cache=qkv["k_cache"], v_cache=qkv["v_cache"], hq=qkv["hq"], hkv=qkv["hkv"])


def linear(x: torch.Tensor, lin: Linear, out: torch.Tensor | None = None,
           residual: torch.Tensor | None = None, out_f32: bool = False, waves: int = 0, splitk: int = 0,
           norm: tuple | None = None, row_idx: torch.Tensor | None = None, qkv: dict | None = None,
           path: int = 0, norm_out: tuple | None = None, prenorm: tuple | None = None,
           ar=None, attn: dict | None = None) -> torch.Tensor:
    """out = epilogue(prologue(x) @ W^T).

    attn (with qkv, decode-only steps): dict(block_tables, context_lens, query_start, out, part_o,
    part_ml, part_size, scale) — the step's decode attention over q = this projection's output, run
    in the projection's launch when the decode kernel takes it (csrc/kernels/qkv_attn.hip), else
    launched right after it; returns q as without it.

    ar (GPU, <= 16 rows, bf16 epilogue): a :class:`vgate.parallel.custom_allreduce.CustomAllReduce`;
    the TP row-parallel GEMM then all-reduces in its epilogue: out = bf16(sum over ranks of
    x @ W^T [+ bias]) + residual, one launch and no copy-in (gemm_epilogue.h epilogue_ar).

    RMSNorm hand-off to the int4 decode kernels (GPU, <= 16 rows, TP = 1; gemm_epilogue.h):
    norm_out=(hg, ssp, gamma) on a residual GEMM also writes hg = out * gamma and per-16-column
    sums of out^2 into ssp; prenorm=(ssp, eps) on an AWQ consumer whose x IS that hg applies the
    row scale from ssp (no gamma loads or x^2 pass in the int4 kernel).

    norm=(w, eps): fused RMSNorm of x rows (deferred row scale, see gemm.hip); row_idx: gather rows of x first
    (GPU: with out_f32 only, the LM head's form — the binding rejects it under another epilogue);
    qkv=dict(positions, slots, cos_sin, k_cache, v_cache, hq, hkv): fused bias + RoPE +
    KV write, returns q [M, hq*128] (layout "qkv" only).
    """
    M = row_idx.numel() if row_idx is not None else x.shape[0]
    silu = lin.layout == "silu"
    if qkv is not None:
        ncols = qkv["hq"] * 128
    else:
        ncols = lin.N // 2 if silu else lin.N
    # CPU reference path: fp32 activations in -> fp32 activations out (the engine's exact CPU mode,
    # EngineConfig.dtype = "float32"); every other caller passes bf16 and gets the kernels' rounding
    act = torch.float32 if not _gpu(x) and x.dtype == torch.float32 else torch.bfloat16
    if out is None:
        out = torch.empty(M, ncols, dtype=torch.float32 if out_f32 else act, device=x.device)
    if not _gpu(x):
        xx = x[row_idx.long()] if row_idx is not None else x
        if norm is not None:
            xx, _ = ref.rmsnorm_ref(xx, norm[0], norm[1])
        wd = lin.dense_weight()
        if silu:
            I = lin.N // 2
            out.copy_(ref.silu_mul_linear_ref(xx, wd[:I], wd[I:], act=act))
        elif qkv is not None:
            y = ref.linear_ref(xx, wd, lin.bias, act=act)
            ref.rope_kv_ref(y, qkv["positions"], qkv["slots"], qkv["cos_sin"], qkv["k_cache"], qkv["v_cache"],
                            qkv["hq"], qkv["hkv"], 128)
            out.copy_(y[:, :ncols])
            if attn is not None:
                _attn_after(out, qkv, attn)
        else:
            out.copy_(ref.linear_ref(xx, wd, lin.bias, residual, out_f32, act=act))
        return out
    C = native()
    epi = EPI_QKV if qkv is not None else EPI_SILU if silu else EPI_F32 if out_f32 else EPI_BF16
    route = _gemm_route(lin, M, waves=waves, splitk=splitk, path=path, row_idx=row_idx, ar=ar, norm_out=norm_out)
    if route[0] == "dequant":
        dq = (_linear_fp8_dequant if lin.kind == "fp8" else _linear_mxfp4_dequant if lin.kind == "mxfp4" else
              _linear_awq_dequant)
        return dq(x, lin, out, residual, norm, qkv, epi, route[1])
    _, path, waves, splitk, ntb = route
    # (fault: the hand-off polls' word, at M > 16 the stream-K prefill kernel's bounded ticket poll)
    kw = dict(bias=lin.bias, res=residual, ws=workspace(x.device), waves=waves, splitk=splitk, ntb=ntb, path=path,
              fault=fault_word(x.device), **_norm_kw(norm, lin.norm_gamma is not None), **_qkv_kw(qkv))
    if M <= 16:  # stream-K slots / the decode split-K granules (zeroed, self-clearing)
        kw["sk_ws"] = sk_workspace(x.device)
    if row_idx is not None:
        kw["row_idx"] = row_idx
    if lin.kind == "awq":
        kw.update(awq_scales=lin.scales, awq_zeros=lin.zeros, group=lin.group)
        if lin.szp is not None:
            kw["awq_szp"] = lin.szp
    if lin.kind in ("fp8", "mxfp4"):
        if prenorm is not None:
            raise ValueError(f"{lin.kind} Linear: no norm hand-off")
        if lin.kind == "fp8":
            kw["fp8_scales"] = lin.fscales
        else:
            kw["mxfp4_scales"] = lin.mscales
        if attn is not None:  # the two-launch form: these kernels take no fused-attention operands
            C.gemm(x, lin.wp, lin.N, lin.K, out, epi, **kw)
            _attn_after(out, qkv, attn)
            return out
    if norm_out is not None:
        kw.update(hg_out=norm_out[0], ssp_out=norm_out[1], hg_gamma=norm_out[2])
    if prenorm is not None:
        kw.update(ssp_in=prenorm[0], eps=float(prenorm[1]))
    if ar is not None:
        if M > 16 or epi != EPI_BF16:
            raise ValueError("fused all-reduce: decode rows (<= 16) and the bf16 epilogue only")
        kw.update(ar_bases=ar.bases, ar_rank=ar.rank, ar_fused_off=ar.fused_off)
    if attn is not None:
        if qkv is None or M > 16:
            raise ValueError("fused attention: the decode QKV projection (qkv epilogue, <= 16 rows)")
        if not FUSE_QKV_ATTN:
            C.gemm(x, lin.wp, lin.N, lin.K, out, epi, **kw)
            _attn_after(out, qkv, attn)
            return out
        kw.update(fa_block_tables=attn["block_tables"], fa_context_lens=attn["context_lens"],
                  fa_query_start=attn["query_start"], fa_out=attn["out"], fa_part_o=attn["part_o"],
                  fa_part_ml=attn["part_ml"], fa_tickets=attn_tickets(x.device), fa_sync=qa_sync(x.device),
                  fa_part_size=int(attn["part_size"]), fa_scale=float(attn["scale"]), fa_dbg_ts=attn.get("dbg_ts"))
    C.gemm(x, lin.wp, lin.N, lin.K, out, epi, **kw)
    return out


def _attn_after(q, qkv, attn):
    """The two-launch form of ``linear(..., attn=...)``: decode attention over the projection's q."""
    if not _gpu(q):
        attention_decode(q, q.stride(0), qkv["k_cache"], qkv["v_cache"], attn["block_tables"], attn["context_lens"],
                         attn["out"], attn["part_o"], attn["part_ml"], qkv["hq"], qkv["hkv"], int(attn["part_size"]),
                         float(attn["scale"]), query_start=attn["query_start"])
        return
    e = torch.empty(0, dtype=torch.int32, device=q.device)
    attention(q, q.stride(0), qkv["k_cache"], qkv["v_cache"], attn["block_tables"], attn["context_lens"],
              attn["query_start"], e, e, attn["out"], attn["part_o"], attn["part_ml"], qkv["hq"], qkv["hkv"],
              int(attn["part_size"]), float(attn["scale"]))


def _linear_awq_dequant(x, lin: Linear, out, residual, norm, qkv, epi, plan_kw: dict):
    """Long AWQ step: int4 -> bf16 fragment-packed scratch (RMSNorm gamma folded in), then the
    bf16 kernels with the row-scale-only RMSNorm mode — same epilogues, no resident bf16 copy."""
    C = native()
    scratch = reserve_awq_scratch(x.device, lin.N * lin.K)[: lin.N * lin.K]
    gamma = norm[0] if norm is not None else None
    C.awq_dequant(lin.wp, lin.scales, lin.zeros, lin.N, lin.K, lin.group, scratch, gamma)
    C.gemm(x, scratch, lin.N, lin.K, out, epi, bias=lin.bias, res=residual, ws=workspace(x.device),
           **_norm_kw(norm, True), **_qkv_kw(qkv), **plan_kw)
    return out


def _linear_fp8_dequant(x, lin: Linear, out, residual, norm, qkv, epi, plan_kw: dict):
    """FP8 step of M > 16 rows: e4m3 -> bf16 fragment-packed scratch (scales and the RMSNorm gamma folded
    in), then the bf16 kernels with the row-scale-only RMSNorm mode; the scratch is the AWQ path's."""
    C = native()
    scratch = reserve_awq_scratch(x.device, lin.N * lin.K)[: lin.N * lin.K]
    gamma = norm[0] if norm is not None else None
    C.fp8_dequant(lin.wp, lin.fscales, lin.N, lin.K, scratch, gamma)
    C.gemm(x, scratch, lin.N, lin.K, out, epi, bias=lin.bias, res=residual, ws=workspace(x.device),
           **_norm_kw(norm, True), **_qkv_kw(qkv), **plan_kw)
    return out


def _linear_mxfp4_dequant(x, lin: Linear, out, residual, norm, qkv, epi, plan_kw: dict):
    """MXFP4 step of M > 16 rows: e2m1 -> bf16 fragment-packed scratch (block scales and the RMSNorm gamma
    folded in), then the bf16 kernels with the row-scale-only RMSNorm mode; the scratch is the AWQ path's."""
    C = native()
    scratch = reserve_awq_scratch(x.device, lin.N * lin.K)[: lin.N * lin.K]
    gamma = norm[0] if norm is not None else None
    C.mxfp4_dequant(lin.wp, lin.mscales, lin.N, lin.K, scratch, gamma)
    C.gemm(x, scratch, lin.N, lin.K, out, epi, bias=lin.bias, res=residual, ws=workspace(x.device),
           **_norm_kw(norm, True), **_qkv_kw(qkv), **plan_kw)
    return out


def attention(q, q_stride, k_cache, v_cache, block_tables, context_lens, query_start, tile_seq, tile_q0, out,
              part_o, part_ml, Hq: int, Hkv: int, part_size: int, scale: float, tickets=None):
    """Unified paged attention for a mixed step (decode rows + prefill tiles, one launch).
    Decode partitions of one (sequence, KV head) are merged in-launch by the last arriving
    block (``tickets``: zeroed int32 [>= S*Hkv], defaults to a per-device buffer)."""
    if tickets is None:
        tickets = attn_tickets(q.device)
    native().attention(q, q_stride, k_cache, v_cache, block_tables, context_lens, query_start, tile_seq, tile_q0,
                       out, part_o, part_ml, Hq, Hkv, part_size, scale, 0, tickets,
                       flash_ws=workspace(q.device) if FLASH_SPLIT else None, fault=fault_word(q.device))
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """y = RMSNorm(x [+ residual]) * w; when residual is given it is updated in place to x + residual."""
    if out is None:
        out = torch.empty_like(x)
    if not _gpu(x):
        y, s = ref.rmsnorm_ref(x, w, eps, residual)
        if residual is not None:
            residual.copy_(s)
        out.copy_(y)
        return out
    native().rmsnorm(x, residual, w, out, eps)
    return out


def embedding(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor | None = None, vstart: int = 0,
              prev: torch.Tensor | None = None):
    """Row gather with vocab-shard masking (rows outside this TP rank's shard are zero).
    ids < 0 name a token the previous step sampled on the device: id = prev[-id - 1]."""
    if out is None:
        out = torch.empty(ids.numel(), table.shape[1], dtype=table.dtype, device=table.device)
    if not _gpu(table):
        if prev is not None and bool((ids < 0).any()):
            ids = torch.where(ids < 0, prev.to(ids.device)[(-ids - 1).clamp(min=0).long()], ids)
        out.copy_(ref.embedding_ref(ids, table, vstart))
        return out
    native().embedding(ids, table, out, vstart, prev)
    return out


def rope_kv(qkv, positions, slots, cos_sin, k_cache, v_cache, Hq: int, Hkv: int, D: int) -> None:
    if not _gpu(qkv):
        ref.rope_kv_ref(qkv, positions, slots, cos_sin, k_cache, v_cache, Hq, Hkv, D)
        return
    native().rope_kv(qkv, positions, slots, cos_sin, k_cache, v_cache, Hq, Hkv, D)


def qk_norm_rope_kv(qkv, positions, slots, cos_sin, q_norm, k_norm, eps: float, k_cache, v_cache, Hq: int, Hkv: int,
                    q_out) -> None:
    """Qwen3 QK-norm behind a plain QKV projection (csrc/kernels/qk_norm.hip): per-head RMSNorm of the
    q / k heads of ``qkv`` [T, (Hq + 2 Hkv) * 128] with ``q_norm`` / ``k_norm`` [128], NeoX RoPE, q ->
    ``q_out`` [>= T, >= Hq * 128], k and v -> the paged cache (slots < 0: q only). ``qkv`` is read only."""
    if not _gpu(qkv):
        ref.qk_norm_rope_kv_ref(qkv, positions, slots, cos_sin, q_norm, k_norm, eps, k_cache, v_cache, Hq, Hkv, 128,
                                q_out)
        return
    native().qk_norm_rope_kv(qkv, positions, slots, cos_sin, q_norm, k_norm, float(eps), k_cache, v_cache, Hq, Hkv,
                             q_out)


def attention_decode(q, q_stride, k_cache, v_cache, block_tables, context_lens, out, part_o, part_ml,
                     Hq: int, Hkv: int, part_size: int, scale: float, query_start=None):
    """One query token per sequence. q rows index = sequence (or query_start[s+1]-1)."""
    if not _gpu(q):
        S = context_lens.numel()
        if query_start is None:
            qs = torch.arange(S + 1, dtype=torch.int32)
        else:
            qs = query_start
        # reference wants only the decode rows
        rows = (qs[1:] - 1).long()
        D = k_cache.shape[-1]
        qq = q.view(q.shape[0], -1)[rows, : Hq * D].reshape(S, Hq, D)
        o = ref.attention_ref(qq, k_cache, v_cache, block_tables, context_lens,
                              torch.arange(S + 1, dtype=torch.int32), Hq, Hkv, scale)
        out.view(out.shape[0], Hq, D)[rows] = o
        return out
    native().attn_decode(q, q_stride, k_cache, v_cache, block_tables, context_lens, query_start, out,
                         part_o, part_ml, Hq, Hkv, part_size, scale)
    return out


def prefill_tiles(query_lens: list[int], lead: int = 32) -> tuple[list[int], list[int]]:
    """16-query prefill tiles (sequence, first query) in the attention kernel's order: see
    :func:`tile_order`."""
    seq, q0 = [], []
    for s, ql in enumerate(query_lens):
        for t in tile_order(ql, lead):
            seq.append(s)
            q0.append(int(t))
    return seq, q0


def flash_lead(hq: int, hkv: int) -> int:
    """Queries per flash-prefill block for a head layout (attention.hip flash_cfg: 8 waves when
    G = hq / hkv divides 8, else 6; two 16-query column tiles per wave up to G = 4, one above;
    the waves are G heads x NW / G query groups). Restated here so that it works without the native
    module; tests/test_attn_probe_gpu.py _has_flash is the third copy: change the three together."""
    G = max(1, hq // max(hkv, 1))
    nw = 8 if 8 % G == 0 else (6 if 6 % G == 0 else 0)
    if nw == 0:
        return 16
    return 16 * (2 if G <= 4 else 1) * (nw // G)


def tile_order(qlen: int, lead: int = 32):
    """First queries of a sequence's 16-query tiles, ordered for the flash prefill kernel: the
    tiles that start a ``lead``-query group (the flash blocks that work; the others exit at once)
    first, longest causal range first, then the rest. The working blocks are then the first ones
    of the grid, spread round-robin over the 8 XCDs, and the longest start first. Correctness
    does not depend on the order (the 16-query kernel is order-free, flash blocks find their
    group from the tile), only the load balance does."""
    import numpy as _np
    t = _np.arange(0, qlen, 16, dtype=_np.int32)[::-1]
    return _np.concatenate([t[t % lead == 0], t[t % lead != 0]])


def attention_prefill(q, q_stride, k_cache, v_cache, block_tables, context_lens, query_start,
                      tile_seq, tile_q0, out, Hq: int, Hkv: int, scale: float):
    if not _gpu(q):
        D = k_cache.shape[-1]
        T = q.shape[0]
        qq = q.view(T, -1)[:, : Hq * D].reshape(T, Hq, D)
        o = ref.attention_ref(qq, k_cache, v_cache, block_tables, context_lens, query_start, Hq, Hkv, scale)
        out.view(T, Hq, D).copy_(o)
        return out
    native().attn_prefill(q, q_stride, k_cache, v_cache, block_tables, context_lens, query_start,
                          tile_seq, tile_q0, out, Hq, Hkv, scale,
                          flash_ws=workspace(q.device) if FLASH_SPLIT else None, fault=fault_word(q.device))
    return out


def sample(logits, temperature=None, top_p=None, top_k=None, seeds=None, offsets=None,
           out=None, out_logprob=None, generators=None):
    """Temperature / top-k / top-p sampling per row (csrc/kernels/sampling.hip)."""
    B = logits.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
    if not _gpu(logits):
        out.copy_(ref.sample_ref(logits, temperature, top_p, top_k, generators))
        return out
    native().sample(logits, temperature, top_p, top_k, seeds, offsets, out, out_logprob, sample_workspace(logits.device),
                    fault_word(logits.device))
    return out


def process_logits(logits, proc_view, prev_tokens=None):
    """Repetition / presence / frequency penalties and logit_bias on the sampled rows before the
    sampler (csrc/kernels/logits_proc.hip; ``proc_view``: vgate.runtime.logits_proc.ProcView).
    GPU: in place, returns ``logits``. CPU: the sparse reference on a COPY, which is returned (the
    caller's logits stay unprocessed)."""
    pv = proc_view
    if not _gpu(logits):
        return ref.process_logits_sparse(logits.clone(), pv.row_off, pv.pend, pv.par, pv.entries, prev_tokens)
    native().process_logits(logits, pv.row_off, pv.pend, pv.par, pv.entries, prev_tokens)
    return logits


LOGPROB_TOP = ref.LOGPROB_TOP
LOGPROB_REC_WORDS = 44  # int32 words of a row's record: {chosen id, logprob, 20 x (id, logprob), 2 pad}


def logprob_views(rec: torch.Tensor):
    """(chosen_lp [S] f32, top_ids [S, 20] i32, top_lp [S, 20] f32) as views of records int32 [S, 44]."""
    top = rec[:, 2: 2 + 2 * LOGPROB_TOP].unflatten(1, (LOGPROB_TOP, 2))
    return rec[:, 1].view(torch.float32), top[:, :, 0], top[:, :, 1].view(torch.float32)


def logprobs(logits, tokens, k_rows, out=None):
    """Per-row log-probabilities after the sampler (csrc/kernels/logprobs.hip, two launches): the
    log-softmax at temperature 1 of fp32 ``logits`` [S, V] as the sampler read them. ``tokens`` [S]
    int32 are the sampled ids, ``k_rows`` [S] int32 the alternatives each row wants (0..20; < 0: the
    row did not ask). Returns (chosen_lp [S] f32, top_ids [S, 20] i32, top_lp [S, 20] f32): the first
    k_rows[r] entries of row r are its most likely tokens by (raw fp32 logit descending, id ascending),
    the rest (-1, 0.0). They are views of ``out``, the rows' records int32 [>= S, 44] (allocated when
    None; ``out[r, 0]`` is the chosen id); rows with k_rows < 0 are left untouched in it.
    CPU: :func:`vgate.ops.reference.logprobs_ref` cast to fp32."""
    S = logits.shape[0]
    if out is None:
        out = torch.zeros(S, LOGPROB_REC_WORDS, dtype=torch.int32, device=logits.device)
    rec = out[:S]
    if _gpu(logits):
        native().logprobs(logits, tokens, k_rows, logprob_partials(logits.device, S), rec)
        return logprob_views(rec)
    lp, ids, tlp = ref.logprobs_ref(logits, tokens, k_rows)
    asked = torch.as_tensor(k_rows).reshape(-1)[:S].cpu() >= 0
    new = torch.zeros(S, LOGPROB_REC_WORDS, dtype=torch.int32)
    new[:, 0] = torch.as_tensor(tokens).reshape(-1)[:S].to(torch.int32).clamp(0, logits.shape[1] - 1)
    c, i, t = logprob_views(new)
    c.copy_(lp.to(torch.float32))
    i.copy_(ids.to(torch.int32))
    t.copy_(tlp.to(torch.float32))
    rec[asked] = new[asked]
    return logprob_views(rec)


def host_device_copy(dst: torch.Tensor, src: torch.Tensor, nbytes: int) -> None:
    """Copy the first ``nbytes`` between a pinned host tensor and a device tensor on the current
    stream. GPU: a kernel on the compute queue (csrc/kernels/elementwise.hip copy16_kernel), so the
    step loop's metadata upload and sampled-id download take no SDMA engine hand-off; both tensors
    must hold ``nbytes`` rounded up to 16 (without the extension: a non-blocking tensor copy)."""
    if (dst.is_cuda or src.is_cuda) and native_available():
        native().kernel_copy(dst, src, int(nbytes))
        return
    d8 = dst.view(torch.uint8) if dst.dtype != torch.uint8 else dst
    s8 = src.view(torch.uint8) if src.dtype != torch.uint8 else src
    d8[:nbytes].copy_(s8[:nbytes], non_blocking=True)


def softmax_scale(head_dim: int) -> float:
    return 1.0 / math.sqrt(head_dim)


__all__ = [
    "native", "native_available", "pack_weight", "unpack_weight", "interleave_gate_up", "pack_awq",
    "Linear", "linear", "attention", "workspace", "fault_word", "reset_handoffs",
    "row_permutation", "reserve_awq_scratch", "pack_awq_sz", "pack_fp8", "unpack_fp8", "pack_mxfp4", "unpack_mxfp4", "pack_mxfp4_scales", "unpack_mxfp4_scales", "mxfp4_dequant_ref", "rmsnorm", "embedding", "rope_kv", "qk_norm_rope_kv", "attention_decode", "attention_prefill",
    "prefill_tiles", "sample", "logprobs", "logprob_views", "softmax_scale", "ref", "host_device_copy", "tune_prefill", "apply_prefill_plans",
]

