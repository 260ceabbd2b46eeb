"""Integer GEMM problems whose expected output is a known bit pattern (helpers of
tests/test_gemm_exact_gpu.py; exercised without a GPU by tests/test_gemm_exact_cpu.py).

bf16 x bf16 products accumulated in fp32 are exact on small integers, whatever the summation order,
K split or tile shape, so the expectation of every problem here is computed once on the CPU in
float64 and a kernel must reproduce it bit for bit. Every quantity a kernel may round to bf16
(x W^T, + bias, + residual) is asserted to stay within BOUND = 256: integers up to 256 are exact in
bf16, so it does not matter where a kernel rounds.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch

BOUND = 256
SENT = 0.71875      # guard / cache sentinel: exact in bf16 and fp32, never an integer
GATE_MIN = 18       # silu(g) == g in fp32 for g >= 18 (exp(-g) < 2^-25)
GUARD = 16          # guard rows before and after every strided view


def weight_density(K: int) -> float:
    """Density of the ternary weight per K (max |x W^T| measured on 64 x 2048 ternary operands:
    K = 512: 72, 1536: 128, 3072: 171 dense; 6144: 112, 8960: 152 at 0.25)."""
    return 1.0 if K <= 3072 else 0.25


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ternary(shape, density: float, g: torch.Generator, nonneg: bool = False) -> torch.Tensor:
    """float64 entries in {-1, 0, 1} ({0, 1} if nonneg), uniform over the set, thinned to `density`."""
    lo = 0 if nonneg else -1
    t = torch.randint(lo, 2, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density).double()
    return t


def bf16_exact(t64: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, asserting nothing is lost."""
    b = t64.to(torch.bfloat16)
    assert torch.equal(b.double(), t64), "value not representable in bf16"
    return b


@dataclass
class Problem:
    kind: str                     # "plain" | "silu" | "qkv"
    M: int
    N: int
    K: int
    x: torch.Tensor               # [M, K] bf16
    w: torch.Tensor               # [N, K] bf16, original row order (AWQ: the exact dequantised matrix)
    bias: torch.Tensor | None = None   # [N] bf16
    res: torch.Tensor | None = None    # [M, N] bf16
    awq: dict | None = None       # qint int32 [N, K], scales / zeros bf16 [K/g, N], group
    qkv: dict | None = None       # positions, slots, cos_sin, hq, hkv, blocks, bs
    exp: dict = field(default_factory=dict)  # float64 expectations

    def check(self) -> None:
        """The preconditions of exactness (CPU, before any launch)."""
        e = self.exp
        assert float(e["prod"].abs().max()) <= BOUND, ("x W^T", float(e["prod"].abs().max()))
        assert torch.equal(e["prod"], e["prod"].round()), "x W^T not integral"
        if self.kind == "silu":
            g, u = e["gate"], e["up"]
            assert bool(((g == 0) | ((g >= GATE_MIN) & (g <= BOUND))).all()), "gate outside {0} + [18, 256]"
            assert bool((g >= GATE_MIN).any()) and bool((g == 0).any())
            assert float(u.abs().max()) <= BOUND
            return
        assert float(e["biased"].abs().max()) <= BOUND, ("+ bias", float(e["biased"].abs().max()))
        if self.kind == "plain":
            assert float(e["full"].abs().max()) <= BOUND, ("+ residual", float(e["full"].abs().max()))
        # the float32 reference computation is exact on these inputs
        assert torch.equal((self.x.float() @ self.w.float().t()).double(), e["prod"])


def _finish_plain(p: Problem) -> Problem:
    prod = p.x.double() @ p.w.double().t()
    biased = prod + (p.bias.double() if p.bias is not None else 0.0)
    full = biased + (p.res.double() if p.res is not None else 0.0)
    p.exp = dict(prod=prod, biased=biased, full=full)
    p.check()
    return p


@functools.lru_cache(maxsize=None)
def dense_problem(M: int, N: int, K: int, bias: bool = True, res: bool = True, seed: int = 0) -> Problem:
    """Ternary x (dense) and W (density per K), bias in [-8, 8], residual in [-32, 32]."""
    g = _gen(1000 * seed + M + 3 * N + 7 * K)
    x = bf16_exact(ternary((M, K), 1.0, g))
    w = bf16_exact(ternary((N, K), weight_density(K), g))
    b = bf16_exact(torch.randint(-8, 9, (N,), generator=g).double()) if bias else None
    r = bf16_exact(torch.randint(-32, 33, (M, N), generator=g).double()) if res else None
    return _finish_plain(Problem("plain", M, N, K, x, w, b, r))


def _awq_from(t: torch.Tensor, z: torch.Tensor, s: torch.Tensor, group: int) -> tuple[dict, torch.Tensor]:
    """t [N, K] integer offsets, z / s [K/group, N] -> (awq dict, exact dequantised bf16 [N, K])."""
    zz = z.t().repeat_interleave(group, dim=1)
    ss = s.t().repeat_interleave(group, dim=1)
    q = t + zz
    assert int(q.min()) >= 0 and int(q.max()) <= 15
    w = bf16_exact((q - zz) * ss)
    bf16_exact(s * z)  # the stored scale * zero
    return dict(qint=q.to(torch.int32), scales=bf16_exact(s), zeros=bf16_exact(z), group=group), w


@functools.lru_cache(maxsize=None)
def awq_problem(M: int, N: int, K: int, group: int = 128, bias: bool = True, res: bool = True,
                seed: int = 0) -> Problem:
    """int4 q = z + t (t ternary, z in 1..14), power-of-two scales in {0.25, 0.5, 1}; x in {-4, 0, 4}
    at density 1/8, so every product is an integer."""
    g = _gen(2000 * seed + M + 3 * N + 7 * K + group)
    G = K // group
    x = bf16_exact(4.0 * ternary((M, K), 0.125, g))
    t = ternary((N, K), weight_density(K), g)
    z = torch.randint(1, 15, (G, N), generator=g).double()
    s = 0.25 * 2.0 ** torch.randint(0, 3, (G, N), generator=g).double()
    awq, w = _awq_from(t, z, s, group)
    b = bf16_exact(torch.randint(-8, 9, (N,), generator=g).double()) if bias else None
    r = bf16_exact(torch.randint(-32, 33, (M, N), generator=g).double()) if res else None
    return _finish_plain(Problem("plain", M, N, K, x, w, b, r, awq=awq))


def _gate_rows(I: int, K: int, lo: int, hi: int, g: torch.Generator) -> torch.Tensor:
    """[I, K] with 4 entries per row in [lo, hi], the rest 0."""
    wg = torch.zeros(I, K, dtype=torch.float64)
    cols = torch.rand(I, K, generator=g).topk(4, dim=1).indices
    wg.scatter_(1, cols, torch.randint(lo, hi + 1, (I, 4), generator=g).double())
    return wg


def _finish_silu(p: Problem) -> Problem:
    I = p.N // 2
    prod = p.x.double() @ p.w.double().t()
    gate, up = prod[:, :I], prod[:, I:]
    p.exp = dict(prod=prod, gate=gate, up=up, out=(gate * up).to(torch.bfloat16))
    p.check()
    return p


@functools.lru_cache(maxsize=None)
def silu_problem(M: int, I: int, K: int, seed: int = 0) -> Problem:
    """Rows [gate; up]: x in {0, 1}, gate rows with 4 entries in [18, 40] (gate = 0 or 18..160), up rows
    ternary; expectation bf16(gate * up), one rounding of an exact fp32 product."""
    g = _gen(3000 * seed + M + 3 * I + 7 * K)
    x = bf16_exact(ternary((M, K), 1.0, g, nonneg=True))
    if M > 1:
        x[0] = 0  # a row whose gates are all 0
    wg = _gate_rows(I, K, GATE_MIN, 40, g)
    wu = ternary((I, K), weight_density(K), g)
    return _finish_silu(Problem("silu", M, 2 * I, K, x, bf16_exact(torch.cat([wg, wu]))))


@functools.lru_cache(maxsize=None)
def awq_silu_problem(M: int, I: int, K: int, seed: int = 0) -> Problem:
    """AWQ rows [gate; up], group 128: x in {0, 4}; gate rows z = 0, s = 1, 4 nibbles in 5..9 per row
    (gate = 0 or 20..144); up rows as awq_problem."""
    g = _gen(4000 * seed + M + 3 * I + 7 * K)
    G = K // 128
    x = bf16_exact(4.0 * ternary((M, K), 0.5, g, nonneg=True))
    if M > 1:
        x[0] = 0
    tg = _gate_rows(I, K, 5, 9, g)
    tu = ternary((I, K), 0.25 * weight_density(K), g)
    z = torch.cat([torch.zeros(G, I, dtype=torch.float64), torch.randint(1, 15, (G, I), generator=g).double()], 1)
    s = torch.cat([torch.ones(G, I, dtype=torch.float64),
                   0.25 * 2.0 ** torch.randint(0, 3, (G, I), generator=g).double()], 1)
    awq, w = _awq_from(torch.cat([tg, tu]), z, s, 128)
    return _finish_silu(Problem("silu", M, 2 * I, K, x, w, awq=awq))


def exact_cos_sin(max_pos: int = 8, D: int = 128, seed: int = 0) -> torch.Tensor:
    """[max_pos, D] f32 (cos | sin) with entries in {0, +1, -1}: position 0 the identity, 1 / 2 / 3 the
    quarter / half / three-quarter turn, the rest a random quarter-turn multiple per frequency."""
    g = _gen(77 + seed)
    half = D // 2
    turns = torch.randint(0, 4, (max_pos, half), generator=g)
    for p in range(min(4, max_pos)):
        turns[p] = p
    c = torch.tensor([1.0, 0.0, -1.0, 0.0])[turns]
    s = torch.tensor([0.0, 1.0, 0.0, -1.0])[turns]
    return torch.cat([c, s], dim=1).float()


def rope_expect(y: torch.Tensor, positions, slots, cos_sin, hq: int, hkv: int, D: int, blocks: int, bs: int):
    """float64 NeoX rotation of the q / k heads of y [T, (hq + 2 hkv) D] and the paged cache it
    leaves behind (sentinel where nothing is written). Returns (rotated y, k_cache, v_cache)."""
    T = y.shape[0]
    half = D // 2
    v3 = y.double().reshape(T, hq + 2 * hkv, D).clone()
    cs = cos_sin.double()[positions.long()]
    c, s = cs[:, None, :half], cs[:, None, half:]
    x1, x2 = v3[:, : hq + hkv, :half].clone(), v3[:, : hq + hkv, half:].clone()
    v3[:, : hq + hkv, :half] = x1 * c - x2 * s
    v3[:, : hq + hkv, half:] = x2 * c + x1 * s
    kc = torch.full((blocks, hkv, bs, D), SENT, dtype=torch.float64)
    vc = kc.clone()
    if slots is not None:
        for t in range(T):
            sl = int(slots[t])
            if sl >= 0:
                kc[sl // bs, :, sl % bs] = v3[t, hq:hq + hkv]
                vc[sl // bs, :, sl % bs] = v3[t, hq + hkv:]
    return v3.reshape(T, -1), kc, vc


def qkv_meta(M: int, blocks: int = 8, bs: int = 16, seed: int = 0) -> dict:
    """Positions over the whole exact table, distinct slots with every third token skipped (-1)."""
    g = _gen(500 + seed + M)
    cs = exact_cos_sin()
    pos = (torch.arange(M) % cs.shape[0]).int()
    slots = torch.randperm(blocks * bs, generator=g)[:M].int()
    slots[1::3] = -1
    if M == 1:
        slots[0] = 5
    return dict(positions=pos, slots=slots, cos_sin=cs, blocks=blocks, bs=bs)


def _finish_qkv(p: Problem) -> Problem:
    m = p.qkv
    prod = p.x.double() @ p.w.double().t()
    biased = prod + (p.bias.double() if p.bias is not None else 0.0)
    rot, kc, vc = rope_expect(biased, m["positions"], m["slots"], m["cos_sin"], m["hq"], m["hkv"], 128,
                              m["blocks"], m["bs"])
    p.exp = dict(prod=prod, biased=biased, q=rot[:, : m["hq"] * 128], k_cache=kc, v_cache=vc)
    p.check()
    return p


@functools.lru_cache(maxsize=None)
def qkv_problem(M: int, hq: int, hkv: int, K: int, awq: bool = False, seed: int = 0) -> Problem:
    """Rows [q; k; v] in heads of 128 with a bias; M <= blocks * bs = 256 tokens."""
    N = (hq + 2 * hkv) * 128
    base = awq_problem(M, N, K, 128, True, False, seed) if awq else dense_problem(M, N, K, True, False, seed)
    meta = qkv_meta(M, blocks=max(8, (M + 15) // 16 + 2), seed=seed)
    meta.update(hq=hq, hkv=hkv)
    return _finish_qkv(Problem("qkv", M, N, K, base.x, base.w, base.bias, None, awq=base.awq, qkv=meta))


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """The norm-wise statistic of the older kernel tests."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-6))


def perturb(p: Problem, n: int, k: int) -> Problem:
    """The same problem with one weight element moved by one (AWQ: one int4 nibble by one); only
    output column n may change."""
    w = p.w.clone()
    awq = None
    if p.awq is not None:
        q = p.awq["qint"].clone()
        q[n, k] += 1 if int(q[n, k]) < 15 else -1
        awq = dict(p.awq, qint=q)
        g = k // p.awq["group"]
        w[n, k] = ((float(q[n, k]) - float(p.awq["zeros"][g, n])) * float(p.awq["scales"][g, n]))
    else:
        w[n, k] = float(w[n, k]) + (1.0 if float(w[n, k]) < 1 else -1.0)
    return Problem(p.kind, p.M, p.N, p.K, p.x, w, p.bias, p.res, awq=awq, qkv=p.qkv)


def active_k(p: Problem, k0: int = 0) -> int:
    """A column k >= k0 in which some row of x is non-zero (so a change of W[:, k] shows)."""
    nz = (p.x.double().abs().sum(0) > 0).nonzero().flatten()
    return int(nz[nz >= k0][0])


def launches(fn, device: str = "cuda") -> list[tuple]:
    """The launch-timeline entries (name, offset, blocks) of the launches ``fn`` makes (GPU tests)."""
    import pytest

    from vgate import ops
    C = ops.native()
    buf = torch.zeros(1 << 17, dtype=torch.int64, device=device)
    C.timeline_start(buf)
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault: nothing more may start on this device in this session
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            pytest.exit(f"GPU fault, session ended: {e}", returncode=3)
        raise
    finally:
        C.timeline_stop()
    return C.timeline_entries()
