"""Closed-form attention probes (helpers of tests/test_attn_probe_gpu.py; proved without a GPU by
tests/test_attn_probe_cpu.py).

A paged KV cache and queries are built so that the expected output of EVERY (token, head) row is known
without any softmax code, and a kernel that reads one key too many, one too few, a wrong page, a wrong
KV head or a wrong table row returns a recognisably different cache row.

Cache (D = 128, BS = 16), sequence s, KV head h, logical position t:
  V[t][d]   = ((31 t + 17 d + 7 h + 13 s) mod 251) - 125      integers, exact in bf16
  K[t][0:2] = (t // 64, t % 64)                               a two-digit position ramp
  K[t][2:]  = r_t, a fixed +-1 code from a seeded generator
Slots of a sequence's last page at t >= ctx continue the K ramp and code and hold V = 240 (finite
poison); every block no table names holds the K row of position max_blocks * 16 and V = 240, and the
table entries past a sequence's pages name one such block. No index is ever out of range.

Probe kinds, qpos = ctx - qlen + i:
  latest    q = (8192, 128, 0...)    score = 128 t scale: ~11.3 logits per position, the last visible
                                     key wins                                     -> V[qpos]
  earliest  q = (-8192, -128, 0...)                                               -> V[0]
  needle p  q = (0, 0, 6 r_p)        the target leads every other key by >= 20 logits  -> V[p]
  uniform   q = 0                    every score 0, every p = 1                   -> mean(V[0..qpos])
Tolerances: |out - V[target]| <= 1 for the one-hot kinds (softmax leakage <= 0.003, P rounded to bf16
<= 2^-8 125 = 0.49, output rounding <= 0.25; any wrong target moves >= 120 of 128 elements by >= 7);
|out - mean| <= 2^-7 |mean| + 2^-7 for uniform (one fp32 divide and the bf16 store).

Assignment: kind = KINDS[(i + hq + round) % 4]. The needle's target is E[((i + hq + round) // 4 +
4 hq) % len(E)], E the row's sorted edge list. (Indexing E by (i + 3 hq + round) differs from the
kind's index by 2 hq, so every needle would get an EVEN index and an edge list of even length would
never see its last entry, qpos, targeted; counting the needles of a head instead walks E one entry
per needle row or round, and the 4 hq offset gives every head its own stretch.)
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

D, BS = 128, 16
SCALE = 1.0 / math.sqrt(D)
POISON_V = 240.0
SENT = 0.71875      # guard rows / untouched output rows: exact in bf16, never produced by a probe
GUARD = 16          # guard rows before and after the output view
KINDS = ("latest", "earliest", "needle", "uniform")
LATEST, EARLIEST, NEEDLE, UNIFORM = range(4)
CODE_SEED = 20
MAX_POS = 1280      # positions the +-1 code covers (contexts stay <= 1100)
NEEDLE_GAIN = 6.0
NEEDLE_GAP = 20.0   # logits between a needle's target and every other key
NEEDLE_STRIDE = 4   # entries of E between the needle targets of neighbouring heads
TOL_ONEHOT = 1.0

LAYOUTS = [(8, 1), (12, 2), (6, 2), (32, 8), (4, 2), (16, 16), (10, 2)]
DECODE_CTXS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 290, 513, 1025]
DECODE_GROUPS = (tuple(DECODE_CTXS[0::2]), tuple(DECODE_CTXS[1::2]))
PARTS = (64, 512, 1024)
DECODE_ROUNDS = 16
# (qlen, ctx); empty sequences inside the list and at its end (the padding of a graph bucket: its
# query_start is the row behind q, which no block may read)
PREFILL_PAIRS = ((1, 1), (15, 15), (16, 16), (17, 17), (33, 70), (0, 0), (64, 64), (65, 101), (63, 300), (130, 130),
                 (70, 330), (0, 0))
MIXED_PAIRS = ((1, 5), (1, 1), (15, 15), (16, 16), (1, 64), (17, 17), (33, 70), (0, 0), (64, 64), (1, 65), (65, 101),
               (63, 300), (1, 700), (130, 130), (70, 330), (0, 0), (0, 0))
MIXED_PARTS = (64, 512)
MIXED_ROUNDS = 4    # every head of a single-query row meets every kind
MUTANTS = ("causal+1", "causal-1", "ctx+1", "drop0", "chunk32", "partition", "table", "kvhead", "swap", "rowlate")


@functools.lru_cache(maxsize=None)
def code() -> torch.Tensor:
    """[MAX_POS + 1, D - 2] float64 of +-1."""
    g = torch.Generator()
    g.manual_seed(CODE_SEED)
    return (torch.randint(0, 2, (MAX_POS + 1, D - 2), generator=g) * 2 - 1).double()


def k_rows(t: torch.Tensor) -> torch.Tensor:
    """K rows [len(t), D] float64 of positions t."""
    t = t.long()
    return torch.cat([(t // 64).double()[:, None], (t % 64).double()[:, None], code()[t]], dim=1)


def v_rows(s: int, h: int, t: torch.Tensor) -> torch.Tensor:
    """V rows [len(t), D] float64 of sequence s, KV head h at positions t (the formula, no poison)."""
    d = torch.arange(D)
    return ((31 * t.long()[:, None] + 17 * d[None, :] + 7 * h + 13 * s) % 251 - 125).double()


def bf16_exact(t64: torch.Tensor) -> torch.Tensor:
    b = t64.to(torch.bfloat16)
    assert torch.equal(b.double(), t64), "value not representable in bf16"
    return b


@dataclass(frozen=True)
class Spec:
    Hq: int
    Hkv: int
    qlens: tuple
    ctxs: tuple
    part: int = 0      # decode partition size (0: a prefill-only case)
    rounds: int = 1
    seed: int = 0
    name: str = "case"


def decode_spec(Hq, Hkv, part, group) -> Spec:
    ctxs = DECODE_GROUPS[group]
    return Spec(Hq, Hkv, (1,) * len(ctxs), ctxs, part, DECODE_ROUNDS, seed=group, name="decode")


def query_start_spec(Hq, Hkv, part) -> Spec:
    """Decode rows at query_start[s + 1] - 1 of a wider q: the sequences of another query length are
    not decode work and their rows keep the sentinel; the last sequence is empty (query_start = T)."""
    return Spec(Hq, Hkv, (1, 3, 1, 0, 1, 1, 2, 1, 0), (65, 40, 513, 0, 17, 290, 64, 128, 0), part, DECODE_ROUNDS, seed=7,
                name="qstart")


def prefill_spec(Hq, Hkv) -> Spec:
    return Spec(Hq, Hkv, tuple(p[0] for p in PREFILL_PAIRS), tuple(p[1] for p in PREFILL_PAIRS), 0, 1, seed=3,
                name="prefill")


def mixed_spec(Hq, Hkv, part) -> Spec:
    return Spec(Hq, Hkv, tuple(p[0] for p in MIXED_PAIRS), tuple(p[1] for p in MIXED_PAIRS), part, MIXED_ROUNDS, seed=5,
                name="mixed")


def all_specs() -> list:
    """Every case the GPU file launches."""
    out = []
    for Hq, Hkv in LAYOUTS:
        for part in PARTS:
            out += [decode_spec(Hq, Hkv, part, g) for g in (0, 1)]
        out.append(query_start_spec(Hq, Hkv, 64))
        out.append(prefill_spec(Hq, Hkv))
        out += [mixed_spec(Hq, Hkv, part) for part in MIXED_PARTS]
    return out


def spec_id(sp: Spec) -> str:
    return f"{sp.name}-{sp.Hq}x{sp.Hkv}-p{sp.part}-s{sp.seed}"


def edges(ctx: int, qlen: int, qpos: int, part: int) -> list:
    e = {0, 15, 16, 31, 32, 63, 64, 127, 128, ctx - qlen - 1, ctx - qlen, qpos - 1, qpos}
    if part > 0:
        e |= {part - 1, part}
    return sorted(x for x in e if 0 <= x <= qpos)


class Case:
    """One built case: cache, tables, queries of every round and the closed-form expectation."""

    def __init__(self, sp: Spec):
        self.spec = sp
        Hq, Hkv = sp.Hq, sp.Hkv
        self.G = G = Hq // Hkv
        self.S = S = len(sp.qlens)
        self.R = R = sp.rounds
        qs = [0]
        for ql in sp.qlens:
            qs.append(qs[-1] + ql)
        self.T = T = qs[-1]
        self.qs = torch.tensor(qs, dtype=torch.int32)
        self.cl = torch.tensor(sp.ctxs, dtype=torch.int32)
        npg = [(c + BS - 1) // BS for c in sp.ctxs]
        self.npg = npg
        self.maxb = maxb = max(npg) + 1
        used = sum(npg)
        self.nblk = nblk = used + 3
        g = torch.Generator()
        g.manual_seed(1000 + sp.seed)
        perm = torch.randperm(nblk, generator=g).tolist()
        if 0 not in perm[:used] and used > 0:  # block 0 belongs to some sequence
            j = perm.index(0)
            perm[0], perm[j] = perm[j], perm[0]
        self.poison_blk = perm[used]
        bt = torch.full((S, maxb), self.poison_blk, dtype=torch.int32)
        kc = k_rows(torch.full((BS,), maxb * BS)).expand(nblk, Hkv, BS, D).clone()
        vc = torch.full((nblk, Hkv, BS, D), POISON_V, dtype=torch.float64)
        at = 0
        for s in range(S):
            ctx = sp.ctxs[s]
            for j in range(npg[s]):
                b = perm[at]
                at += 1
                bt[s, j] = b
                t = torch.arange(j * BS, (j + 1) * BS)
                kc[b] = k_rows(t)[None]
                n = min(BS, ctx - j * BS)
                for h in range(Hkv):
                    vc[b, h, :n] = v_rows(s, h, t[:n])
        self.bt = bt
        self.kc, self.vc = bf16_exact(kc), bf16_exact(vc)
        # per token: sequence, index in it, position
        self.tok_seq = torch.zeros(T, dtype=torch.long)
        self.tok_i = torch.zeros(T, dtype=torch.long)
        self.qpos = torch.zeros(T, dtype=torch.long)
        for s in range(S):
            a, b = qs[s], qs[s + 1]
            self.tok_seq[a:b] = s
            self.tok_i[a:b] = torch.arange(b - a)
            self.qpos[a:b] = sp.ctxs[s] - (b - a) + torch.arange(b - a)
        q = torch.zeros(R, T, Hq, D, dtype=torch.float64)
        exp = torch.zeros(R, T, Hq, D, dtype=torch.float64)
        # edge lists, one row per token (padded), then every (round, token, head) at once
        E = [edges(sp.ctxs[s], sp.qlens[s], qp, sp.part) for s, qp in zip(self.tok_seq.tolist(), self.qpos.tolist())]
        elen = torch.tensor([len(e) for e in E], dtype=torch.long)
        epad = torch.tensor([e + [0] * (16 - len(e)) for e in E], dtype=torch.long).reshape(T, 16)
        hqs = torch.arange(Hq)[None, None, :]
        n = torch.arange(R)[:, None, None] + self.tok_i[None, :, None] + hqs  # [R, T, Hq]
        self.kind = n % 4
        idx = (n // 4 + NEEDLE_STRIDE * hqs) % elen[None, :, None]
        tg = epad[torch.arange(T)[None, :, None].expand_as(idx), idx]
        tg = torch.where(self.kind == LATEST, self.qpos[None, :, None].expand_as(tg), tg)
        tg = torch.where(self.kind == EARLIEST, torch.zeros_like(tg), tg)
        self.target = torch.where(self.kind == UNIFORM, torch.full_like(tg, -1), tg)
        sign = torch.tensor([1.0, -1.0, 0.0, 0.0], dtype=torch.float64)[self.kind]
        q[..., 0] = 8192.0 * sign
        q[..., 1] = 128.0 * sign
        nd = self.kind == NEEDLE
        q[..., 2:][nd] = NEEDLE_GAIN * code()[self.target[nd]]
        for s in range(S):
            a, b = qs[s], qs[s + 1]
            if b == a or sp.ctxs[s] <= 0:
                continue
            pos = torch.arange(sp.ctxs[s])
            for h in range(Hkv):
                V = v_rows(s, h, pos)
                pm = V.cumsum(0) / (pos + 1).double()[:, None]
                hsl = slice(h * G, (h + 1) * G)
                tg = self.target[:, a:b, hsl]
                e = V[tg.clamp(min=0)]
                um = pm[self.qpos[a:b]][None, :, None, :].expand(R, b - a, G, D)
                exp[:, a:b, hsl] = torch.where((tg < 0)[..., None], um, e)
        self.q = bf16_exact(q).reshape(R, T, Hq * D)
        self.expected = exp
        uni = (self.kind == UNIFORM)[..., None]
        self.tol = torch.where(uni, exp.abs() * 2.0 ** -7 + 2.0 ** -7, torch.full_like(exp, TOL_ONEHOT))
        live = torch.tensor([sp.qlens[s] > 0 and sp.ctxs[s] > 0 for s in range(S)])
        dec = torch.tensor([sp.qlens[s] == 1 for s in range(S)])
        self.live = live[self.tok_seq] if T else torch.zeros(0, dtype=torch.bool)
        self.live_decode = (live & dec)[self.tok_seq] if T else torch.zeros(0, dtype=torch.bool)

    def row_desc(self, t: int, hq: int, r: int) -> str:
        kd = KINDS[int(self.kind[r, t, hq])]
        return f"seq {int(self.tok_seq[t])} token {int(self.tok_i[t])} head {hq} kind {kd}"


@functools.lru_cache(maxsize=None)
def build(sp: Spec) -> Case:
    return Case(sp)


# --------------------------------------------------------------------------- float64 reference
def attention64(q, kc, vc, bt, cl, qs, Hq, Hkv, scale, mutate=None, part=0, seqs=None, fill=0.0):
    """Plain float64 paged causal attention, one row at a time over an explicit visible set.
    q [R, T, Hq * D] (or [T, Hq * D]); returns [R, T, Hq, D] float64; rows of sequences without
    queries or context hold ``fill``. ``mutate`` names one wrong kernel (MUTANTS), applied to the
    sequences in ``seqs`` (default: every sequence the mutation can touch)."""
    assert mutate is None or mutate in MUTANTS
    if q.dim() == 2:
        q = q[None]
    R, T = q.shape[0], q.shape[1]
    G = Hq // Hkv
    S = cl.numel()
    maxb = bt.shape[1]
    q = q.double().reshape(R, T, Hq, D)
    out = torch.full((R, T, Hq, D), fill, dtype=torch.float64)
    qsl, cll = qs.tolist(), cl.tolist()
    livs = [s for s in range(S) if qsl[s + 1] > qsl[s] and cll[s] > 0]
    bt = bt.clone()
    on = (lambda s: True) if seqs is None else (lambda s: s in seqs)
    if mutate == "swap":
        a, b = livs[0], livs[1]
        bt[[a, b]] = bt[[b, a]]
    if mutate == "table":
        s = next(s for s in livs if cll[s] > BS and on(s))
        bt[s, 0] = bt[s, 1]
    hmap = torch.arange(Hq) // G
    if mutate == "kvhead":
        hmap[0] = (hmap[0] + 1) % Hkv
    for s in livs:
        a, b = qsl[s], qsl[s + 1]
        ql, ctx = b - a, cll[s]
        mut = mutate if on(s) else None
        n = min(ctx + 1, maxb * BS) if mut == "ctx+1" else ctx
        pages = bt[s, : (n + BS - 1) // BS].long()
        K = kc[pages].double().permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :n]
        V = vc[pages].double().permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :n]
        sc = torch.einsum("rqhd,htd->rqht", q[:, a:b], K[hmap]) * scale
        qpos = ctx - ql + torch.arange(ql)
        bound = qpos
        if mut == "causal+1":
            bound = (qpos + 1).clamp(max=ctx - 1)
        elif mut == "causal-1":
            bound = qpos - 1
        elif mut == "ctx+1":
            bound = qpos + 1
        vis = torch.arange(n)[None, :] <= bound[:, None]  # [ql, n]
        if mut == "drop0":
            vis[:, 0] = False
        elif mut == "chunk32":
            vis[:, 31:33] = False
        elif mut == "partition" and ql == 1 and part > 0 and ctx > part:
            vis[:, part: 2 * part] = False
        sc = sc.masked_fill(~vis[None, :, None, :], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        p = torch.where(vis.any(1)[None, :, None, None], p, torch.zeros_like(p))  # no visible key: l = 0 -> 0
        out[:, a:b] = torch.einsum("rqht,htd->rqhd", p, V[hmap])
    if mutate == "rowlate":
        t = qsl[livs[0]]  # the first live row lands one row late (the caller's buffer has guard rows)
        late = out[:, t].clone()
        out[:, t] = float("nan")  # marker: the caller leaves this row untouched
        return out, (t + 1, late)
    return out


def mutant_exists(sp: Spec, mutate: str) -> bool:
    live = [(ql, c) for ql, c in zip(sp.qlens, sp.ctxs) if ql > 0 and c > 0]
    if mutate == "causal+1":
        return any(ql >= 2 for ql, _ in live)
    if mutate == "chunk32":
        return any(c - 1 >= 32 for _, c in live)
    if mutate == "partition":
        return sp.part > 0 and any(ql == 1 and c > sp.part for ql, c in live)
    if mutate == "table":
        return any(c > BS for _, c in live)
    if mutate == "kvhead":
        return sp.Hkv > 1
    if mutate == "swap":
        return len(live) >= 2
    return bool(live)


def ref64(case: Case, mutate=None) -> torch.Tensor:
    """The float64 reference of a case in the launch buffer's shape [R, GUARD + T + GUARD, Hq * D]
    (guards and rows without work = SENT)."""
    sp = case.spec
    buf = torch.full((case.R, case.T + 2 * GUARD, sp.Hq * D), SENT, dtype=torch.float64)
    res = attention64(case.q, case.kc, case.vc, case.bt, case.cl, case.qs, sp.Hq, sp.Hkv, SCALE, mutate, sp.part,
                      fill=SENT)
    late = None
    if mutate == "rowlate":
        res, late = res
    res = res.reshape(case.R, case.T, -1)
    res = torch.where(torch.isnan(res), torch.full_like(res, SENT), res)
    buf[:, GUARD:GUARD + case.T] = res
    if late is not None:
        buf[:, GUARD + late[0]] = late[1].reshape(case.R, -1)
    return buf


# --------------------------------------------------------------------------- check + diagnosis
STATS: dict = {}  # path -> {"rows", "onehot" (largest |out - expected| / tolerance), "uniform"}


def _search_order(case: Case, s0: int, h0: int):
    """(sequence, KV head) pairs, the row's own first: V rows repeat across (s, h, t) (31 t + 7 h + 13 s
    mod 251), and among equal candidates the diagnosis names the one in the row's own sequence and head."""
    sp = case.spec
    pairs = [(s, h) for s in range(case.S) for h in range(sp.Hkv) if sp.ctxs[s] > 0]
    return sorted(pairs, key=lambda p: (p[0] != s0, p[1] != h0, p))


def _nearest_row(case: Case, row: torch.Tensor, s0: int, h0: int):
    """(max |diff|, what) of the cache row nearest to ``row`` over all slots of all sequences."""
    sp = case.spec
    best = (float("inf"), "")
    for s, h in _search_order(case, s0, h0):
        d = (v_rows(s, h, torch.arange(sp.ctxs[s])) - row[None]).abs().amax(1)
        j = int(d.argmin())
        if float(d[j]) < best[0]:
            best = (float(d[j]), (s, h, j))
    for val, name in ((POISON_V, "poison 240"), (SENT, "the untouched sentinel"), (0.0, "zeros")):
        d = float((row - val).abs().max())
        if d < best[0] or (d <= TOL_ONEHOT and name != "zeros"):
            best = (d, name)
    return best


def _nearest_mean(case: Case, row: torch.Tensor, s0: int, h0: int):
    """Nearest mean of positions a..b (a in {0, 1}; the slots of the last page past ctx count as the
    poison they hold) over all sequences and KV heads."""
    sp = case.spec
    best = (float("inf"), None)
    for s, h in _search_order(case, s0, h0):
        n = case.npg[s] * BS
        pos = torch.arange(n)
        V = v_rows(s, h, pos)
        V[sp.ctxs[s]:] = POISON_V
        cs = torch.cat([torch.zeros(1, D, dtype=torch.float64), V.cumsum(0)])
        for a in (0, 1):
            cnt = (pos + 1 - a).clamp(min=1).double()[:, None]
            m = (cs[1:] - cs[a]) / cnt
            d = (m - row[None]).abs().amax(1)
            d[:a] = float("inf")
            j = int(d.argmin())
            if float(d[j]) < best[0]:
                best = (float(d[j]), (s, h, a, j))
    return best


def diagnose(case: Case, r: int, t: int, hq: int, row: torch.Tensor) -> str:
    s, h = int(case.tok_seq[t]), hq // case.G
    diff = float((row - case.expected[r, t, hq]).abs().max()) if not torch.isnan(row).any() else float("nan")
    head = case.row_desc(t, hq, r)
    if torch.isnan(row).any() or torch.isinf(row).any():
        return f"{head}: expected position {int(case.target[r, t, hq])}, got NaN / Inf"
    if int(case.kind[r, t, hq]) == UNIFORM:
        qp = int(case.qpos[t])
        d, who = _nearest_mean(case, row, s, h)
        dr, what = _nearest_row(case, row, s, h)
        if isinstance(what, str) and what != "zeros" and dr <= TOL_ONEHOT:
            got = what
        elif not bool(row.any()):
            got = "zeros"
        elif who is None:
            got = "nothing recognisable"
        else:
            s2, h2, a, b = who
            got = f"nearest mean of positions {a}..{b} of seq {s2}" + (f" kv head {h2}" if (s2, h2) != (s, h) else "")
            got += f" (off it by {d:.3g})"
        return f"{head}: expected mean of positions 0..{qp}, got {got} (max |diff| {diff:.3g})"
    d, what = _nearest_row(case, row, s, h)
    if isinstance(what, str):
        got = what
    else:
        s2, h2, j = what
        got = f"position {j} of seq {s2}" + (f" kv head {h2}" if h2 != h else "")
        if d > TOL_ONEHOT:
            got = f"no single cache row (nearest: {got}, off it by {d:.3g})"
    return f"{head}: expected position {int(case.target[r, t, hq])}, got {got} (max |diff| {diff:.3g})"


def check(case: Case, buf: torch.Tensor, path: str | None = None, decode_only: bool = False) -> dict:
    """Every element of every row of a launch buffer [R, GUARD + T + GUARD, Hq * D] (or one round
    without the leading axis) against the closed form; guards and rows without work must hold SENT.
    Raises AssertionError with a decoded diagnosis; returns the observed margins."""
    sp = case.spec
    if buf.dim() == 2:
        buf = buf[None]
    R, T = case.R, case.T
    assert buf.shape == (R, T + 2 * GUARD, sp.Hq * D), buf.shape
    buf = buf.detach().cpu().double()
    guards = torch.cat([buf[:, :GUARD], buf[:, GUARD + T:]], dim=1)
    bad = (guards != SENT).any(-1).nonzero()
    if len(bad):
        r, g = bad[0].tolist()
        row = (g - GUARD) if g < GUARD else (T + g - GUARD)
        raise AssertionError(f"{spec_id(sp)} round {r}: guard row {row} (relative to the output view) was written")
    out = buf[:, GUARD:GUARD + T].reshape(R, T, sp.Hq, D)
    live = case.live_decode if decode_only else case.live
    dead = ~live
    if dead.any():
        wr = (out[:, dead] != SENT).any(-1).any(-1).nonzero()
        if len(wr):
            r, k = wr[0].tolist()
            t = int(dead.nonzero()[k])
            raise AssertionError(f"{spec_id(sp)} round {r}: row {t} (seq {int(case.tok_seq[t])}, no work in this "
                                 f"launch) was written")
    if not live.any():
        return {"rows": 0, "onehot": 0.0, "uniform": 0.0}
    o, e, tol, kind = out[:, live], case.expected[:, live], case.tol[:, live], case.kind[:, live]
    err = (o - e).abs()
    frac = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / tol).amax(-1)  # [R, L, Hq]
    fail = frac > 1.0
    if fail.any():
        lines = []
        tl = live.nonzero().flatten()
        for kd in range(4):
            w = (fail & (kind == kd)).nonzero()
            if len(w):
                r, k, hq = w[0].tolist()
                lines.append(diagnose(case, r, int(tl[k]), hq, out[r, int(tl[k]), hq]) + (f" [round {r}]" if R > 1 else ""))
        raise AssertionError(f"{spec_id(sp)}: {int(fail.sum())} of {fail.numel()} rows outside the closed form\n  "
                             + "\n  ".join(lines))
    uni = kind == UNIFORM
    res = {"rows": int(fail.numel()),
           "onehot": float(frac[~uni].max()) if (~uni).any() else 0.0,
           "uniform": float(frac[uni].max()) if uni.any() else 0.0}
    if path is not None:
        st = STATS.setdefault(path, {"rows": 0, "onehot": 0.0, "uniform": 0.0})
        st["rows"] += res["rows"]
        st["onehot"] = max(st["onehot"], res["onehot"])
        st["uniform"] = max(st["uniform"], res["uniform"])
    return res


def needle_gaps(case: Case) -> float:
    """Smallest (target logit - largest other visible logit) over every needle row of a case."""
    c = code()
    best = float("inf")
    nd = (case.kind == NEEDLE).nonzero()
    if not len(nd):
        return best
    tg = case.target[nd[:, 0], nd[:, 1], nd[:, 2]]
    qp = case.qpos[nd[:, 1]]
    corr = c[tg] @ c[: int(qp.max()) + 1].T  # [N, P]
    pos = torch.arange(corr.shape[1])[None, :]
    other = corr.masked_fill((pos > qp[:, None]) | (pos == tg[:, None]), float("-inf")).amax(1)
    other = torch.where(torch.isinf(other), torch.full_like(other, -float(D)), other)  # a single visible key
    gap = (float(D - 2) - other) * NEEDLE_GAIN * SCALE
    return float(gap.min())
