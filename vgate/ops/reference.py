"""Pure-PyTorch fp32 reference implementations of every vgate kernel.

Two roles:
  * numerics oracle for the HIP kernels (tests compare GPU kernels against these),
  * the CPU execution path, so the whole engine (scheduler, KV manager, sampler
    bookkeeping, HTTP stack) runs and is tested on a machine without a GPU.

They are deliberately written for clarity, not speed.
"""
from __future__ import annotations

import math

import torch


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None):
    """Returns (y, new_residual). Mirrors HF RMSNorm rounding (normalise in f32, cast, scale)."""
    if residual is not None:
        s = (x.float() + residual.float()).to(x.dtype)
    else:
        s = x
    xf = s.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = ((xf * inv).to(x.dtype).float() * w.float()).to(x.dtype)
    return y, (s if residual is not None else None)


def embedding_ref(ids: torch.Tensor, table: torch.Tensor, vstart: int = 0) -> torch.Tensor:
    local = ids.long() - vstart
    ok = (local >= 0) & (local < table.shape[0])
    out = table[local.clamp(0, table.shape[0] - 1)]
    return out * ok.unsqueeze(-1).to(out.dtype)


def linear_ref(x: torch.Tensor, w: torch.Tensor, bias=None, residual=None, out_f32=False, act=torch.bfloat16):
    """``act``: activation dtype the result is rounded to (bf16 mirrors the kernels' epilogues;
    float32 = the CPU engine's exact mode, EngineConfig.dtype)."""
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if out_f32:
        return y
    y = y.to(act)
    if residual is not None:
        y = (y.float() + residual.float()).to(act)
    return y


def silu_mul_linear_ref(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, act=torch.bfloat16) -> torch.Tensor:
    g = x.float() @ w_gate.float().t()
    u = x.float() @ w_up.float().t()
    return (torch.nn.functional.silu(g) * u).to(act)


def rope_cos_sin(max_pos: int, dim: int, theta: float, scaling: dict | None = None,
                 device="cpu") -> torch.Tensor:
    """[max_pos, dim] f32 table: first half cos, second half sin (NeoX layout)."""
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling.get("factor", 8.0)
        lo = scaling.get("low_freq_factor", 1.0)
        hi = scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    elif scaling and scaling.get("rope_type", scaling.get("type")) == "linear":
        inv = inv / scaling.get("factor", 1.0)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def rope_kv_ref(qkv, positions, slots, cos_sin, k_cache, v_cache, Hq, Hkv, D):
    """In-place NeoX rotary on q,k of `qkv` [T, (Hq+2Hkv)*D]; writes k,v to the paged cache."""
    T = qkv.shape[0]
    if T == 0:
        return
    v3 = qkv.view(T, Hq + 2 * Hkv, D)
    half = D // 2
    cs = cos_sin[positions.long()]  # [T, D]
    c, s = cs[:, None, :half], cs[:, None, half:]
    qk = v3[:, : Hq + Hkv].float()
    x1, x2 = qk[..., :half], qk[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    v3[:, : Hq + Hkv] = rot
    if slots is None:
        return
    BS = k_cache.shape[2]
    sl = slots.long()
    ok = sl >= 0
    if ok.any():
        idx = torch.nonzero(ok).squeeze(-1)
        blk, off = sl[idx] // BS, sl[idx] % BS
        k_cache[blk, :, off] = v3[idx, Hq:Hq + Hkv]
        v_cache[blk, :, off] = v3[idx, Hq + Hkv:]


def qk_norm_rope_kv_ref(qkv, positions, slots, cos_sin, q_norm, k_norm, eps, k_cache, v_cache, Hq, Hkv, D, q_out):
    """Qwen3 QK-norm: RMSNorm over each q / k head's D dims (weights q_norm / k_norm [D]), then NeoX
    rotary; q -> q_out[:, :Hq*D], k and the unchanged v -> the paged cache (slots < 0: q only). fp32
    from the inputs to one rounding to qkv.dtype (fp32 activations: nothing rounds); qkv is not modified."""
    T = qkv.shape[0]
    if T == 0:
        return
    v3 = qkv.view(T, Hq + 2 * Hkv, D)
    half = D // 2
    x = v3[:, : Hq + Hkv].float()
    gamma = torch.cat([q_norm.float().reshape(1, D).expand(Hq, D), k_norm.float().reshape(1, D).expand(Hkv, D)])
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gamma
    cs = cos_sin[positions[:T].long()]  # [T, D]
    c, s = cs[:, None, :half], cs[:, None, half:]
    n1, n2 = n[..., :half], n[..., half:]
    rot = torch.cat([n1 * c - n2 * s, n2 * c + n1 * s], dim=-1).to(qkv.dtype)
    q_out[:T, : Hq * D] = rot[:, :Hq].reshape(T, Hq * D)
    if slots is None:
        return
    BS = k_cache.shape[2]
    sl = slots[:T].long()
    ok = sl >= 0
    if ok.any():
        idx = torch.nonzero(ok).squeeze(-1)
        blk, off = sl[idx] // BS, sl[idx] % BS
        k_cache[blk, :, off] = rot[idx, Hq:].to(k_cache.dtype)
        v_cache[blk, :, off] = v3[idx, Hq + Hkv:].to(v_cache.dtype)


def _gather_kv(cache, table_row, n):
    BS = cache.shape[2]
    nb = (n + BS - 1) // BS
    blocks = table_row[:nb].long()
    kv = cache[blocks]  # [nb, H, BS, D]
    return kv.permute(1, 0, 2, 3).reshape(cache.shape[1], nb * BS, cache.shape[3])[:, :n]


def attention_ref(q, k_cache, v_cache, block_tables, context_lens, query_start, Hq, Hkv, scale):
    """Varlen causal attention over the paged cache. q: [T, Hq, D] (any row stride).

    query_start: [S+1] cumulative query counts (decode: arange(S+1)).
    Returns [T, Hq, D] in q.dtype.
    """
    T = q.shape[0]
    D = q.shape[-1]
    out = torch.zeros(T, Hq, D, dtype=q.dtype, device=q.device)
    G = Hq // Hkv
    qs = query_start.tolist()
    cl = context_lens.tolist()
    for s in range(len(cl)):
        a, b = qs[s], qs[s + 1]
        ql, ctx = b - a, cl[s]
        if ql <= 0 or ctx <= 0:
            continue
        K = _gather_kv(k_cache, block_tables[s], ctx).float()  # [Hkv, ctx, D]
        V = _gather_kv(v_cache, block_tables[s], ctx).float()
        K = K.repeat_interleave(G, dim=0)
        V = V.repeat_interleave(G, dim=0)
        qq = q[a:b].float().transpose(0, 1)  # [Hq, ql, D]
        sc = (qq @ K.transpose(1, 2)) * scale  # [Hq, ql, ctx]
        qpos = torch.arange(ctx - ql, ctx, device=q.device)[:, None]
        kpos = torch.arange(ctx, device=q.device)[None, :]
        sc = sc.masked_fill(kpos > qpos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[a:b] = (p @ V).transpose(0, 1).to(q.dtype)
    return out


def sample_ref(logits, temperature, top_p, top_k, generators=None):
    """Reference sampler (sort based). Returns int32 [B]."""
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.int32)
    for i in range(B):
        row = logits[i].float()
        t = float(temperature[i]) if temperature is not None else 0.0
        if t <= 1e-5:
            out[i] = int(torch.argmax(row))
            continue
        probs = torch.softmax(row / t, dim=-1)
        sp, si = torch.sort(probs, descending=True)
        keep = torch.ones_like(sp, dtype=torch.bool)
        k = int(top_k[i]) if top_k is not None else -1
        if 0 < k < V:
            keep[k:] = False
        p = float(top_p[i]) if top_p is not None else 1.0
        if p < 1.0:
            csum = torch.cumsum(sp, 0)
            excl = csum - sp
            keep &= excl < p
        sp = sp * keep
        g = generators[i] if generators is not None else None
        j = torch.multinomial(sp.cpu(), 1, generator=g)
        out[i] = int(si[j])
    return out


def awq_dequant_ref(qint: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, group: int):
    """qint: [N, K] int (0..15); scales/zeros: [K/group, N] -> bf16 [N, K] weight (w = (q - z) * s)."""
    N, K = qint.shape
    s = scales.float().t().repeat_interleave(group, dim=1)  # [N, K]
    z = zeros.float().t().repeat_interleave(group, dim=1)
    return ((qint.float() - z) * s).to(torch.bfloat16)


# ----------------------------------------------------------------------------- logits processors
def _penalise(x, cnt, in_prompt, bias, par):
    """The sparse path's arithmetic on gathered fp32 values: par = {rep, inv_rep, pres, freq} as fp32
    scalars (inv_rep comes from the host, as the kernel reads it), every step one rounded operation."""
    rep, inv_rep, pres, freq = par[0], par[1], par[2], par[3]
    if float(rep) != 1.0:
        seen = in_prompt | (cnt > 0)
        x = torch.where(seen, torch.where(x > 0, x * inv_rep, x * rep), x)
    x = x - freq * cnt.to(torch.float32)
    x = torch.where(cnt > 0, x - pres, x)
    return x + bias


def process_logits_ref(logits: torch.Tensor, prompt_ids, output_ids, params) -> torch.Tensor:
    """Dense oracle of the logits processors for ONE row ``logits`` [V] (fp32): counts by bincount
    over the whole vocabulary, then the penalty / bias steps on every element. ``output_ids`` includes
    every token generated so far (the in-flight one too). Returns a new tensor."""
    x = logits.detach().float().cpu().clone()
    V = x.numel()
    out = torch.as_tensor(list(output_ids), dtype=torch.int64)
    prm = torch.as_tensor(list(prompt_ids), dtype=torch.int64)
    cnt = torch.bincount(out[(out >= 0) & (out < V)], minlength=V)
    in_prompt = torch.bincount(prm[(prm >= 0) & (prm < V)], minlength=V) > 0
    bias = torch.zeros(V, dtype=torch.float32)
    for t, b in params.logit_bias.items():
        if 0 <= int(t) < V:
            bias[int(t)] = float(b)
    f32 = torch.float32
    rep = torch.tensor(params.repetition_penalty, dtype=f32)
    if float(rep) != 1.0:  # 1. repetition: prompt and output tokens
        inv_rep = torch.tensor(1.0, dtype=f32) / rep
        x = torch.where(in_prompt | (cnt > 0), torch.where(x > 0, x * inv_rep, x * rep), x)
    x = x - torch.tensor(params.frequency_penalty, dtype=f32) * cnt.to(f32)  # 2. frequency: product, then difference
    x = torch.where(cnt > 0, x - torch.tensor(params.presence_penalty, dtype=f32), x)  # 3. presence
    return x + bias  # 4. bias


def process_logits_sparse(logits: torch.Tensor, row_off, pend, par, entries, prev=None) -> torch.Tensor:
    """The logits kernel's algorithm on the host, in place on ``logits`` [S, V] fp32 (CPU): row r's
    unique-token entries {tok, cnt (bit 31 = in prompt), bias bits, pad} are
    entries[row_off[r]: row_off[r + 1]], par[r] = {rep, inv_rep, pres, freq}, pend[r] = 0 or
    -(slot + 1) of the sequence's in-flight token in ``prev``."""
    S, V = logits.shape
    row_off = torch.as_tensor(row_off).tolist()
    pend = torch.as_tensor(pend).tolist()
    par = torch.as_tensor(par).reshape(-1, 4)
    entries = torch.as_tensor(entries).reshape(-1, 4)
    for r in range(S):
        a, b = max(row_off[r], 0), min(row_off[r + 1], entries.shape[0])
        p = -1
        if pend[r] < 0 and prev is not None:
            slot = min(max(-(pend[r] + 1), 0), prev.numel() - 1)
            p = int(prev[slot])
            if not 0 <= p < V:
                p = -1
        if b <= a and p < 0:
            continue
        e = entries[a:b] if b > a else entries[:0]
        tok = e[:, 0].to(torch.int64)
        word = e[:, 1].to(torch.int64)
        cnt = word & 0x7FFFFFFF
        in_prompt = word < 0
        bias = e[:, 2].contiguous().view(torch.float32)
        ok = (tok >= 0) & (tok < V)
        tok, cnt, in_prompt, bias = tok[ok], cnt[ok], in_prompt[ok], bias[ok]
        if p >= 0:
            hit = tok == p
            if bool(hit.any()):
                cnt = cnt + hit.to(cnt.dtype)
            else:
                tok = torch.cat([tok, torch.tensor([p])])
                cnt = torch.cat([cnt, torch.tensor([1])])
                in_prompt = torch.cat([in_prompt, torch.tensor([False])])
                bias = torch.cat([bias, torch.zeros(1)])
        row = logits[r]
        row[tok] = _penalise(row[tok], cnt, in_prompt, bias, par[r].float())
    return logits


# ------------------------------------------------------------------------------------ logprobs
LOGPROB_TOP = 20  # alternatives per row (csrc/kernels/launchers.h)


def rank_keys(logits: torch.Tensor) -> torch.Tensor:
    """int64 keys whose descending order is the logprob ranking of fp32 ``logits`` [..., V]: the raw
    fp32 value descending, ties (-0.0 == 0.0 included) to the lower token id. Exact and unique."""
    x = logits.detach().to(torch.float32).cpu() + 0.0  # -0.0 -> 0.0: equal values get equal bits
    b = x.contiguous().view(torch.int32).to(torch.int64)
    mono = torch.where(b >= 0, b, -(b & 0x7FFFFFFF) - 1)  # monotone in the float's value
    ids = torch.arange(x.shape[-1], dtype=torch.int64)
    return mono * (1 << 32) + ((1 << 31) - 1 - ids)


def logprobs_ref(logits: torch.Tensor, tokens, k_rows):
    """Oracle of the logprob kernels for fp32 ``logits`` [S, V]: a float64 log-softmax, the chosen
    token's value (``tokens`` clamped into [0, V)), and per row the min(k_rows, 20) most likely tokens
    ranked by the RAW fp32 logits (descending, ties to the lower id; :func:`rank_keys`), not by the
    computed log-probabilities. Returns (chosen_lp [S] f64, top_ids [S, 20] i64, top_lp [S, 20] f64);
    entries beyond a row's k are (-1, 0.0), and a row with k < 0 is all (-1, 0.0) with chosen_lp 0."""
    x = logits.detach().to(torch.float32).cpu()
    S, V = x.shape
    tok = torch.as_tensor(tokens).to(torch.int64).cpu().reshape(-1)[:S].clamp(0, V - 1)
    k = torch.as_tensor(k_rows).to(torch.int64).cpu().reshape(-1)[:S]
    lp = torch.log_softmax(x.to(torch.float64), dim=-1)
    n = min(LOGPROB_TOP, V)
    order = torch.topk(rank_keys(x), n, dim=-1).indices  # keys are unique: the order is exact
    chosen = lp.gather(1, tok[:, None])[:, 0]
    top_ids = torch.full((S, LOGPROB_TOP), -1, dtype=torch.int64)
    top_lp = torch.zeros(S, LOGPROB_TOP, dtype=torch.float64)
    top_ids[:, :n] = order
    top_lp[:, :n] = lp.gather(1, order)
    off = torch.arange(LOGPROB_TOP)[None, :] >= k.clamp(max=LOGPROB_TOP)[:, None]
    top_ids[off] = -1
    top_lp[off] = 0.0
    chosen = torch.where(k < 0, torch.zeros_like(chosen), chosen)
    return chosen, top_ids, top_lp
