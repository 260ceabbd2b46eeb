"""Shared cases of the sampler tests: a float64 numpy oracle of csrc/kernels/sampling.hip, draw by
draw, and named cases (padded logits, per-row parameters, the oracle's results), built once.

The noise is integer-exact (Philox4x32-10, then ((c >> 9) + 0.5) * 2^-23), so the oracle has every
uniform of the kernel bit for bit. Everything after it is an argmax of keys and an accept test; the
oracle evaluates both in float64 and flags a row `ambiguous` when a decision on its path was closer
than fp32 can resolve:

  key gap    the two best keys of a pass differ by <= tau_a + tau_b, tau_i = 2^-20 (|x_i|/T + |L_i| + 1).
             The device key is fma(x, fl(1/T), -L), L = logf(fmaxf(-logf(u), 1e-30f)): logf is 1 ulp
             (ROCm HIP math), the outer log turns the inner relative error into 2^-23 absolute, so the
             key is off by <= 2^-23 (1.5 |x|/T + 1.5 |L| + 1); tau is about 5x that. Elements with the
             same (x, u) have bit-equal keys on the device too: an exact tie, lowest index wins.
  mass band  |q - top_p Z| <= (V/256 + 64) 2^-24 Z: one thread adds at most V/256 terms in sequence (one
             block per row), 64 ulp for term error, rescales and the merge trees. A threshold <= 0 and
             an empty set above the candidate (q = 0 exactly) are decided exactly in any precision.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

GUARD = 1e30           # columns [V, ldl) of the padded buffer: never read by the sampler
PAD = 64
MAX_ROUNDS = 60        # sampling_common.h SAMPLE_MAX_ROUNDS
GRAN_ROWS = 128        # launchers.h SAMPLE_GRAN_ROWS
NSEG_CAPS = (1, 2, 7, 33, 64)
SEEDS = (0, 1, 2 ** 32, -1, -2 ** 63 + 5)
OFFSETS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)
TEMPS = (0.0, 1e-6, 0.3, 0.7, 1.0, 1.5, 100.0)
TOP_PS = (0.3, 0.5, 0.9, 0.999999, 1.0)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def top_ks(V: int):
    return (-1, 0, 1, 2, 20, 50, V - 1, V, V + 5)


def segments(B: int, V: int, cap: int = 64) -> int:
    """Blocks per row of the launch (sampling.hip sample_segments / launch_sample)."""
    if B > GRAN_ROWS:
        return 1
    return max(1, min(256 // max(B, 1), cap, (V // 4) // 256))


def v_lo(V: int, nseg: int, s: int) -> int:
    """First float4 of segment s."""
    return (V // 4) * s // nseg


# ------------------------------------------------------------------------------------ noise
def philox4x32_10(ctr, key):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: ctr (4 arrays), key (2 arrays)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def _u64(a):
    return np.atleast_1d(np.asarray(a, dtype=np.int64)).view(np.uint64)


def uniforms(seed, offset, V: int, round: int) -> np.ndarray:
    """The kernel's uniforms of one pass, float64 [N, V] (each exactly an fp32 value): counter
    {i4, offset_lo, round, offset_hi ^ 0x9E3779B9}, key {seed_lo, seed_hi}, element 4 * i4 + j is
    word j. seed / offset: int64 scalars or [N], reinterpreted as uint64."""
    seed, offset = _u64(seed)[:, None], _u64(offset)[:, None]
    i4 = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    ctr = (i4, offset & _LO, np.uint64(round), (offset >> _S32) ^ _W0)
    w = philox4x32_10(ctr, (seed & _LO, seed >> _S32))
    w = np.stack(np.broadcast_arrays(*w), axis=-1).reshape(seed.shape[0], -1)[:, :V]
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


# ------------------------------------------------------------------------------------ oracle
def _draw(s, mask, seed, offset, rnd):
    """Gumbel-max over mask: (winner or -1 [n], ambiguous [n]). s = x / T float64 [n, V]."""
    n, V = s.shape
    u = uniforms(seed, offset, V, rnd)
    L = np.log(np.maximum(-np.log(u), 1e-30))
    key = np.where(mask, s - L, -np.inf)
    rows = np.arange(n)
    w = np.argmax(key, axis=1)  # first occurrence: lowest index
    none = ~mask.any(axis=1)
    with np.errstate(invalid="ignore"):
        tau = 2.0 ** -20 * (np.abs(np.where(mask, s, 0.0)) + np.abs(L) + 1.0)
    same = (s == s[rows, w][:, None]) & (u == u[rows, w][:, None])  # bit-equal keys on the device
    key2 = np.where(same, -np.inf, key)
    r = np.argmax(key2, axis=1)
    two = ~none & (key2[rows, r] > -np.inf)  # a runner-up exists
    with np.errstate(invalid="ignore"):
        ratio = np.where(two, (key[rows, w] - key2[rows, r]) / (tau[rows, w] + tau[rows, r]), np.inf)
    return np.where(none, -1, w), two & (ratio <= 1.0), ratio


@dataclass
class Oracle:
    token: np.ndarray      # [N] int64
    rounds: np.ndarray     # [N] rejection rounds run (mode-1 passes)
    ambiguous: np.ndarray  # [N] bool
    gap_ratio: np.ndarray  # [N] smallest key gap / (tau_a + tau_b) on the row's path (inf: no draw)


def oracle_rows(x, T, top_k, top_p, seed, offset) -> Oracle:
    """The sampler's semantics (top of sampling.hip) in float64 for N rows at once: x [N, V] fp32
    values (finite or -inf), per-row T / top_p (fp32 values), top_k, seed, offset [N]."""
    x32 = np.asarray(x, dtype=np.float32)
    xd = x32.astype(np.float64)
    N, V = xd.shape
    T32 = np.broadcast_to(np.asarray(T, dtype=np.float32), (N,))
    k = np.broadcast_to(np.asarray(top_k, dtype=np.int64), (N,))
    p32 = np.broadcast_to(np.asarray(top_p, dtype=np.float32), (N,))
    seed = np.broadcast_to(np.asarray(seed, dtype=np.int64), (N,))
    offset = np.broadcast_to(np.asarray(offset, dtype=np.int64), (N,))
    greedy = ~(T32 > np.float32(1e-5))
    finite = xd > -np.inf
    amx = np.argmax(xd, axis=1)  # lowest index; 0 for a row without a finite logit
    use_k = (k > 0) & (k < V)
    use_p = p32 < np.float32(1.0)
    token = amx.astype(np.int64).copy()
    rounds = np.zeros(N, dtype=np.int64)
    amb = np.zeros(N, dtype=bool)
    ratio = np.full(N, np.inf)
    act = np.nonzero(~greedy & finite.any(axis=1))[0]
    if act.size == 0:
        return Oracle(token, rounds, amb, ratio)
    s = xd[act] / T32[act].astype(np.float64)[:, None]
    cand, a, g = _draw(s, finite[act], seed[act], offset[act], 0)
    amb[act] |= a
    ratio[act] = np.minimum(ratio[act], g)
    e = np.exp(s - s.max(axis=1, keepdims=True))  # exp(-inf) = 0
    Z = e.sum(axis=1)
    thr = p32[act].astype(np.float64) * Z
    band = (V / 256 + 64) * 2.0 ** -24 * Z
    live = (use_k | use_p)[act] & (cand >= 0)  # rows still testing a candidate
    for rnd in range(1, MAX_ROUNDS + 1):
        i = np.nonzero(live)[0]
        if i.size == 0:
            break
        gi = act[i]
        xj = xd[gi, cand[i]]
        gt = xd[gi] > xj[:, None]
        cnt = gt.sum(axis=1)
        q = np.where(gt, e[i], 0.0).sum(axis=1)
        ok_k = ~use_k[gi] | (cnt < k[gi])
        ok_p = ~use_p[gi] | (q < thr[i])
        close = use_p[gi] & ok_k & (thr[i] > 0) & (cnt > 0) & (np.abs(q - thr[i]) <= band[i])
        amb[gi] |= close
        rounds[gi] = rnd
        rej = ~(ok_k & ok_p)
        live[i[~rej]] = False
        if rej.any():
            ir = i[rej]
            nxt, a, g = _draw(s[ir], gt[rej], seed[act[ir]], offset[act[ir]], rnd)
            amb[act[ir]] |= a & (nxt >= 0)
            ratio[act[ir]] = np.minimum(ratio[act[ir]], g)
            cand[ir] = nxt
            live[ir] = nxt >= 0
    token[act] = np.where(cand >= 0, cand, amx[act])
    return Oracle(token, rounds, amb, ratio)


def oracle_row(x, T, top_k, top_p, seed, offset):
    """One row: (token, rejection rounds, ambiguous)."""
    o = oracle_rows(np.asarray(x, dtype=np.float32)[None, :], T, top_k, top_p, seed, offset)
    return int(o.token[0]), int(o.rounds[0]), bool(o.ambiguous[0])


def support(x, T, top_k, top_p, slack: bool = False) -> np.ndarray:
    """bool [V]: the tokens a sampled (non-greedy) row may return: finite, strictly-greater count
    < top_k and strictly-greater mass < fp32(top_p) Z (float64); the argmax alone if that set is empty.
    slack: the mass threshold plus the mass band, for rows whose decision fp32 cannot resolve."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    V = xd.shape[0]
    keep = xd > -np.inf
    if not keep.any():
        keep[:] = False
        keep[0] = True
        return keep
    s = xd / float(np.float32(T))
    e = np.exp(s - s.max())
    order = np.argsort(-xd, kind="stable")
    xs, es = xd[order], e[order]
    first = np.concatenate([[True], xs[1:] != xs[:-1]])  # first of each group of equal values
    start = np.maximum.accumulate(np.where(first, np.arange(V), 0))
    cnt_gt = np.empty(V, dtype=np.int64)
    cnt_gt[order] = start
    csum = np.concatenate([[0.0], np.cumsum(es)])
    mass_gt = np.empty(V)
    mass_gt[order] = csum[start]
    if 0 < int(top_k) < V:
        keep &= cnt_gt < int(top_k)
    if np.float32(top_p) < np.float32(1.0):
        Z = e.sum()
        thr = float(np.float32(top_p)) * Z + ((V / 256 + 64) * 2.0 ** -24 * Z if slack else 0.0)
        keep &= mass_gt < thr
    if not keep.any():
        keep[int(np.argmax(xd))] = True
    return keep


def target(x, T, top_k, top_p) -> np.ndarray:
    """The exact distribution of a sampled row: float64 softmax at T over support(), renormalised."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    s = xd / float(np.float32(T))
    e = np.where(support(x, T, top_k, top_p), np.exp(s - s[xd > -np.inf].max()), 0.0)
    return e / e.sum()


def logprob_ref(x, T, ids) -> np.ndarray:
    """float64 log_softmax(x / T)[ids] per row (T = 1 for greedy rows): what out_logprob holds, the
    tempered and unfiltered distribution."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    T32 = np.asarray(T, dtype=np.float32)
    Td = np.where(T32 > np.float32(1e-5), T32, np.float32(1.0)).astype(np.float64)
    s = xd / Td[:, None]
    m = s.max(axis=1)
    lse = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    return s[np.arange(xd.shape[0]), np.asarray(ids, dtype=np.int64)] - lse


# ------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    V: int
    B: int
    ldl: int
    nseg: int                  # segments per row at the default cap
    exact: bool                # the result does not depend on fp32 arithmetic: no ambiguous row allowed
    buf: torch.Tensor          # [B, ldl] fp32 (CPU): logits, then GUARD columns
    temperature: torch.Tensor  # [B] fp32
    top_k: torch.Tensor        # [B] int32
    top_p: torch.Tensor        # [B] fp32
    seeds: torch.Tensor        # [B] int64
    offsets: torch.Tensor      # [n_off, B] int64: one launch per row of it
    token: np.ndarray          # [n_off, B] the oracle's results, left unchanged by the tests
    rounds: np.ndarray
    ambiguous: np.ndarray
    gap_ratio: np.ndarray

    @property
    def x(self) -> np.ndarray:
        return self.buf[:, : self.V].numpy()


def _hot_edges(V: int, B: int):
    idx = {0, V - 1}
    for cap in (64,) + NSEG_CAPS:
        n = segments(B, V, cap)
        for s_ in range(1, n):
            idx |= {4 * v_lo(V, n, s_) - 1, 4 * v_lo(V, n, s_)}
    return sorted(idx)


def _fill(kind: str, V: int, B: int, g: torch.Generator):
    """(x [B, V], T, top_k, top_p [B], exact) of a case kind; seeds and offsets are set by build_case."""
    T = torch.ones(B)
    tk = torch.full((B,), -1, dtype=torch.int32)
    tp = torch.ones(B)
    x = torch.empty(B, V)
    exact = False
    r = torch.arange(B)
    if kind in ("equal", "strided"):  # 3a: the winner is the largest uniform, tolerance-free
        x[:] = ((r % 4).float() * 0.5 - 0.5)[:, None]
        if kind == "strided":
            for b in range(B):
                hole = torch.ones(V, dtype=torch.bool)
                hole[b % 37:: 37] = False
                x[b, hole] = float("-inf")
        exact = True
    elif kind == "general":  # 3b: every parameter value, mixed per row
        x = torch.randn(B, V, generator=g) * torch.where(r % 2 == 0, 3.0, 0.8)[:, None]
        sh = (V // 4 + B) % 63
        ks = top_ks(V)
        for b in range(B):
            i = b + sh
            T[b] = TEMPS[i % 7]
            tk[b] = ks[(i + i // 7) % 9]
            tp[b] = TOP_PS[(i + i // 63) % 5]
    elif kind.startswith("chain"):  # 3c: near-uniform rows, the chain climbs ~log V rounds
        for b in range(B):
            x[b] = torch.randperm(V, generator=g).float() * 2.0 ** -10
        T[:] = 100.0
        if kind == "chain_k1":
            tk[:] = 1
            exact = True
        elif kind == "chain_k3":
            tk[:] = 3
        else:
            tp[:] = 0.001
    elif kind == "ties":  # 3d: multiples of 0.5; top_k cuts a tie group, top_p ends inside one
        x = torch.round(torch.randn(B, V, generator=g) * 3 * 2) / 2
        for b in range(B):
            T[b] = (0.7, 1.0, 1.5)[b % 3]
            xs = np.sort(x[b].numpy().astype(np.float64))[::-1]
            inside = np.nonzero(xs[1:] == xs[:-1])[0] + 1  # k with xs[k - 1] == xs[k]
            if b % 3 != 1:
                tk[b] = int(inside[inside >= 5 + b][0])
            if b % 3 != 0:  # half way through the mass of a group of >= 2 equal values near the top
                e = np.exp((xs - xs[0]) / float(T[b]))
                vals, n_eq = np.unique(xs, return_counts=True)
                v = vals[::-1][2 + b % 4:][n_eq[::-1][2 + b % 4:] >= 2][0]
                above, grp = e[xs > v].sum(), e[xs == v].sum()
                tp[b] = float((above + 0.5 * grp) / e.sum())
    elif kind == "edges":  # 3e: hot tokens on both sides of every segment boundary
        x[:] = -30.0
        hot = _hot_edges(V, B)
        for b in range(B):
            x[b, hot] = torch.rand(len(hot), generator=g) * 3
            tk[b] = (20, -1, 7, 20)[b % 4]
            tp[b] = (0.9, 0.9, 1.0, 0.5)[b % 4]
    elif kind == "logprob":  # 3f: filters on, T in {0.7, 1, 1.5}
        x = torch.randn(B, V, generator=g) * torch.where(r % 2 == 0, 3.0, 0.8)[:, None]
        for b in range(B):
            T[b] = (0.7, 1.0, 1.5)[b % 3]
            tk[b] = (50, -1, 20)[b % 3]
            tp[b] = (0.9, 0.5, 1.0, 0.9)[b % 4]
    elif kind == "topp0":  # 3g: q < 0 never holds, the chain runs out: the argmax
        x = torch.randn(B, V, generator=g) * 3
        tp[:] = 0.0
        T[:] = torch.tensor([(1.0, 0.7, 1.5)[b % 3] for b in range(B)])
        tk[:] = torch.tensor([(-1, 20)[b % 2] for b in range(B)], dtype=torch.int32)
    elif kind == "masked":  # 3h: rows without a finite logit among ordinary rows
        x = torch.randn(B, V, generator=g) * 3
        for b in range(B):
            T[b] = (0.7, 0.0, 1.0)[b % 3]
            tk[b] = (20, -1)[b % 2]
            tp[b] = (0.9, 1.0, 0.5)[(b // 2) % 3]
        x[masked_rows(B)] = float("-inf")
    else:
        raise KeyError(kind)
    return x, T, tk, tp, exact


def masked_rows(B: int):
    return [b for b in (1, 3, 6, 129) if b < B] if B > 1 else [0]


# name -> (kind, V, B, launches). Big vocabularies keep B <= 8 and few launches (the oracle costs
# ~30 ms per row and round at V = 65540); B = 130 runs one block per row and stays at V <= 8196.
CASES = {
    "equal-1024x8": ("equal", 1024, 8, 5),
    "equal-1024x130": ("equal", 1024, 130, 5),
    "equal-2052x8": ("equal", 2052, 8, 5),
    "equal-65540x3": ("equal", 65540, 3, 5),
    "equal-151936x8": ("equal", 151936, 8, 5),
    "strided-8196x8": ("strided", 8196, 8, 5),
    "strided-65540x3": ("strided", 65540, 3, 5),
    "general-1024x3": ("general", 1024, 3, 3),
    "general-1024x130": ("general", 1024, 130, 2),
    "general-2052x1": ("general", 2052, 1, 5),
    "general-2052x8": ("general", 2052, 8, 3),
    "general-8196x8": ("general", 8196, 8, 3),
    "general-8196x130": ("general", 8196, 130, 2),
    "general-65540x3": ("general", 65540, 3, 3),
    "general-128256x3": ("general", 128256, 3, 2),
    "general-151936x8": ("general", 151936, 8, 2),
    "chain_k1-8192x8": ("chain_k1", 8192, 8, 2),
    "chain_k3-8192x8": ("chain_k3", 8192, 8, 2),
    "chain_p-8192x8": ("chain_p", 8192, 8, 2),
    "chain_k3-8192x130": ("chain_k3", 8192, 130, 1),
    "ties-2052x8": ("ties", 2052, 8, 3),
    "ties-8196x130": ("ties", 8196, 130, 2),
    "edges-8196x8": ("edges", 8196, 8, 3),
    "edges-65540x3": ("edges", 65540, 3, 3),
    "logprob-2052x8": ("logprob", 2052, 8, 2),
    "logprob-8196x130": ("logprob", 8196, 130, 1),
    "logprob-151936x8": ("logprob", 151936, 8, 1),
    "topp0-8196x8": ("topp0", 8196, 8, 2),
    "topp0-8196x130": ("topp0", 8196, 130, 1),
    "masked-8196x8": ("masked", 8196, 8, 2),
    "masked-8196x130": ("masked", 8196, 130, 1),
}
EXACT_KINDS = ("equal", "strided", "chain_k1")


@functools.lru_cache(maxsize=None)
def build_case(name: str, seed: int = 0) -> Case:
    kind, V, B, n_off = CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + B + 131 * list(CASES).index(name))
    ldl = V + PAD
    x, T, tk, tp, exact = _fill(kind, V, B, g)
    buf = torch.full((B, ldl), GUARD, dtype=torch.float32)
    buf[:, :V] = x
    if exact:  # 3a: every (seed, offset) pair of the two lists within rows 0..4
        seeds = torch.tensor([SEEDS[b % 5] for b in range(B)], dtype=torch.int64)
        offsets = torch.tensor([[OFFSETS[(b + o + b // 5) % 5] for b in range(B)] for o in range(n_off)],
                               dtype=torch.int64)
    else:
        seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, (B,), generator=g, dtype=torch.int64)
        seeds[::3] = torch.arange(0, B, 3) * 7 + 3  # small seeds, as the engine's counters
        offsets = torch.randint(0, 2 ** 44, (n_off, B), generator=g, dtype=torch.int64)
        offsets[0] = torch.arange(B) % 4  # small offsets: the first steps of a request
    res = [oracle_rows(x.numpy(), T.numpy(), tk.numpy(), tp.numpy(), seeds.numpy(), o.numpy()) for o in offsets]
    return Case(name, V, B, ldl, segments(B, V), exact, buf, T, tk, tp, seeds, offsets,
                np.stack([r.token for r in res]), np.stack([r.rounds for r in res]),
                np.stack([r.ambiguous for r in res]), np.stack([r.gap_ratio for r in res]))
