"""Shared pieces of tests/test_qwen3_cpu.py and tests/test_qwen3_gpu.py: the float64 formula of the
QK-norm + RoPE + KV-write op written from its definition (not through vgate.ops.reference), its inputs,
and the engine prompts (those of tests/test_engine_gpu.py)."""
from __future__ import annotations

import torch

import gemm_exact as X

D = 128
HALF = 64
EPS = 1e-6
BS = 16
PROMPTS = {f"q{i}": [3 + (i * 31 + j * 17) % 500 for j in range(7 + 9 * i)] for i in range(6)}


def margin_ok(row: torch.Tensor, tok: int) -> bool:
    """The project's teacher-forcing margin: the token is the reference argmax or within bf16 rounding of it."""
    return bool(row[tok] >= row.max() - 0.05 * row.std())


def make_case(T: int, Hq: int, Hkv: int, seed: int = 0, exact_table: bool = False, dtype=torch.bfloat16):
    """Inputs of one op call: qkv [T, (Hq + 2 Hkv) * 128], distinct non-constant q_norm / k_norm in
    [0.5, 4] (no symmetry between the halves), positions over the table, slots from a permutation with
    every fourth token unwritten (-1)."""
    g = X._gen(9000 + seed + 7 * T + 31 * Hq + 131 * Hkv)
    blocks = (T + BS - 1) // BS + 2
    qkv = (1.5 * torch.randn(T, (Hq + 2 * Hkv) * D, generator=g)).to(dtype)
    qn = (0.5 + 3.5 * torch.rand(D, generator=g)).to(torch.bfloat16)
    kn = (0.5 + 3.5 * torch.rand(D, generator=g)).to(torch.bfloat16)
    if exact_table:
        cs = X.exact_cos_sin(8, D)
        pos = (torch.arange(T) % 8).int()
    else:
        from vgate.ops.reference import rope_cos_sin
        cs = rope_cos_sin(64, D, 1e4)
        pos = ((torch.arange(T) * 5 + 3) % 64).int()
    slots = torch.randperm(blocks * BS, generator=g)[:T].int()
    slots[2::4] = -1
    return dict(T=T, Hq=Hq, Hkv=Hkv, qkv=qkv, q_norm=qn, k_norm=kn, cos_sin=cs, positions=pos, slots=slots,
                blocks=blocks)


def expect64(c: dict, eps: float = EPS) -> dict:
    """float64, from the definition: per head inv = rsqrt(mean(x^2) + eps), n = x * inv * gamma (q_norm for
    the q heads, k_norm for the k heads), then (n_i, n_{i+64}) -> (n_i c - n_{i+64} s, n_{i+64} c + n_i s).
    Returns q [T, Hq, 128], k [T, Hkv, 128], v, ``cancel`` = |a c| + |b s| per rotated element (the size of
    the two products whose sum is rounded), and the caches a call leaves behind (sentinel where unwritten)."""
    T, Hq, Hkv = c["T"], c["Hq"], c["Hkv"]
    x = c["qkv"].double().reshape(T, Hq + 2 * Hkv, D)
    out = torch.empty(T, Hq + Hkv, D, dtype=torch.float64)
    cancel = torch.empty_like(out)
    for t in range(T):
        cs = c["cos_sin"][int(c["positions"][t])].double()
        co, si = cs[:HALF], cs[HALF:]
        for h in range(Hq + Hkv):
            gamma = (c["q_norm"] if h < Hq else c["k_norm"]).double()
            xh = x[t, h]
            inv = 1.0 / torch.sqrt((xh * xh).sum() / D + eps)
            n = xh * inv * gamma
            a, b = n[:HALF], n[HALF:]
            out[t, h, :HALF] = a * co - b * si
            out[t, h, HALF:] = b * co + a * si
            cancel[t, h, :HALF] = (a * co).abs() + (b * si).abs()
            cancel[t, h, HALF:] = (b * co).abs() + (a * si).abs()
    v = x[:, Hq + Hkv:]
    kc = torch.full((c["blocks"], Hkv, BS, D), X.SENT, dtype=torch.float64)
    vc = kc.clone()
    for t in range(T):
        sl = int(c["slots"][t])
        if sl >= 0:
            kc[sl // BS, :, sl % BS] = out[t, Hq:]
            vc[sl // BS, :, sl % BS] = v[t]
    return dict(q=out[:, :Hq], k=out[:, Hq:], v=v, cancel_q=cancel[:, :Hq], cancel_k=cancel[:, Hq:], k_cache=kc,
                v_cache=vc)


def within(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    err = (got.detach().cpu().double() - want64).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist(),
                                 float((err / bound.clamp_min(1e-300)).max()))


def written(c: dict) -> torch.Tensor:
    """Token indices whose slot is written."""
    return (c["slots"] >= 0).nonzero().flatten()


def cache_rows(cache: torch.Tensor, c: dict) -> torch.Tensor:
    """[n written tokens, Hkv, 128] rows of a paged cache at the written tokens' slots."""
    sl = c["slots"][written(c)].long()
    return cache[sl // BS, :, sl % BS]
