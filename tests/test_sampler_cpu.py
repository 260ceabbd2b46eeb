"""The sampler oracle (tests/sampler_cases.py) on its own, no GPU: Philox known answers, the
uniforms' range, the distribution of its draws against the exact filtered softmax, its support
against vgate.ops.reference.sample_ref, and the share of rows of every case whose decisions fp32
cannot resolve (the GPU tests compare every other row exactly)."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
from vgate.ops import reference as ref


def _words(*w):
    return [np.array([v], dtype=np.uint64) for v in w]


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = sc.philox4x32_10(_words(*ctr), _words(*key))
    assert tuple(int(g[0]) for g in got) == want


def test_uniforms_follow_the_counter_layout():
    """uniforms() is Philox at counter {i4, offset_lo, round, offset_hi ^ 0x9E3779B9}, key {seed_lo,
    seed_hi}, word j to element 4 * i4 + j; int64 seeds are reinterpreted as uint64; every word of the
    seed, the offset and the round reaches the noise."""
    seed, off, rnd, V = -2 ** 63 + 5, 2 ** 40 + 3, 7, 22
    u = sc.uniforms(seed, off, V, rnd)
    assert u.shape == (1, V)
    for i4 in (0, 3, 5):
        w = sc.philox4x32_10(_words(i4, (2 ** 40 + 3) & 0xffffffff, rnd, (2 ** 8) ^ 0x9E3779B9), _words(5, 2 ** 31))
        for j in range(4):
            if 4 * i4 + j < V:
                assert u[0, 4 * i4 + j] == ((int(w[j][0]) >> 9) + 0.5) * 2.0 ** -23
    base = sc.uniforms(3, 9, 64, 1)
    for other in (sc.uniforms(3 + 2 ** 32, 9, 64, 1), sc.uniforms(3, 9 + 2 ** 32, 64, 1), sc.uniforms(3, 9, 64, 2),
                  sc.uniforms(4, 9, 64, 1), sc.uniforms(3, 10, 64, 1)):
        assert (other != base).mean() > 0.9
    both = sc.uniforms(np.array([3, -1]), np.array([9, 2 ** 32]), 64, 1)  # rows are independent calls
    assert np.array_equal(both[0], base[0]) and np.array_equal(both[1], sc.uniforms(-1, 2 ** 32, 64, 1)[0])


def test_uniforms_lie_strictly_inside_the_unit_interval():
    u = sc.uniforms(np.arange(8), np.arange(8) * 2 ** 33, 1 << 16, 0)
    assert u.min() > 0.0 and u.max() < 1.0
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # each exactly an fp32 value
    top = ((0xffffffff >> 9) + 0.5) * 2.0 ** -23
    assert top == 1 - 2.0 ** -24 and float(np.float32(top)) == top
    assert ((0 >> 9) + 0.5) * 2.0 ** -23 == 2.0 ** -24


# ------------------------------------------------------------------------------------ semantics
def test_oracle_rules_on_small_rows():
    x = np.array([0.5, 2.0, -np.inf, 2.0, 1.0, -np.inf, 0.0, 1.5], dtype=np.float32)
    for T in (0.0, 1e-6, 1e-5):  # greedy iff not (T > 1e-5f): the lowest-index argmax, no noise
        assert sc.oracle_row(x, T, -1, 1.0, 5, 9) == (1, 0, False)
    toks = set()
    for off in range(300):
        t, rounds, _ = sc.oracle_row(x, 1.0, -1, 1.0, 11, off)
        assert rounds == 0 and np.isfinite(x[t])
        toks.add(t)
    assert toks == {0, 1, 3, 4, 6, 7}  # every finite token, never a masked one
    for off in range(100):
        assert sc.oracle_row(x, 1.0, 1, 1.0, 11, off)[0] in (1, 3)  # top_k = 1 keeps the whole tie
        assert sc.oracle_row(x, 1.0, 2, 1.0, 11, off)[0] in (1, 3)  # 7 has two tokens above it
        assert sc.oracle_row(x, 1.0, 3, 1.0, 11, off)[0] in (1, 3, 7)
        t, rounds, amb = sc.oracle_row(x, 1.0, -1, 0.0, 11, off)    # top_p = 0: the chain runs out
        assert (t, amb) == (1, False) and rounds >= 1
        for k in (0, -1, 8, 13):                                     # top_k off
            assert sc.oracle_row(x, 1.0, k, 1.0, 11, off)[0] == sc.oracle_row(x, 1.0, -1, 1.0, 11, off)[0]
    none = np.full(8, -np.inf, dtype=np.float32)
    for T, k, p in ((0.0, -1, 1.0), (1.0, -1, 1.0), (0.7, 3, 0.5)):
        assert sc.oracle_row(none, T, k, p, 1, 2) == (0, 0, False)


def test_equal_logits_pick_the_largest_uniform():
    V = 4096
    for seed, off in zip(sc.SEEDS, sc.OFFSETS):
        u = sc.uniforms(seed, off, V, 0)[0]
        assert sc.oracle_row(np.full(V, 1.5, dtype=np.float32), 1.0, -1, 1.0, seed, off)[0] == int(np.argmax(u))


def test_exact_tie_of_keys_is_not_ambiguous():
    """Two elements with the same logit and the same uniform have bit-equal device keys."""
    V = 256
    u = sc.uniforms(1, 2, V, 0)[0]
    assert len(np.unique(u)) == V
    o = sc.oracle_rows(np.zeros((1, V), dtype=np.float32), 1.0, -1, 1.0, 1, 2)
    assert not o.ambiguous[0] and np.isfinite(o.gap_ratio[0]) and o.gap_ratio[0] > 1


# ------------------------------------------------------------------------------------ distribution
def _dist_row(kind):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, generator=g) * 1.5).numpy()
    if kind == "ties":
        x = np.round(x * 2) / 2
    if kind == "holes":
        x[3::5] = -np.inf
    return x.astype(np.float32)


N_DRAWS = 50_000


@pytest.mark.parametrize("kind,T,k,p", [
    ("plain", 1.0, -1, 1.0), ("plain", 0.7, -1, 1.0), ("plain", 1.5, 10, 1.0), ("plain", 1.0, -1, 0.8),
    ("plain", 1.5, 12, 0.6), ("ties", 1.0, 9, 0.85), ("holes", 1.2, 20, 0.9), ("holes", 1.0, -1, 1.0),
], ids=["T1", "T0.7", "topk", "topp", "topk+topp", "ties", "holes-filtered", "holes"])
def test_oracle_draws_follow_the_exact_distribution(kind, T, k, p):
    x = _dist_row(kind)
    q = sc.target(x, T, k, p)
    o = sc.oracle_rows(np.broadcast_to(x, (N_DRAWS, 64)), T, k, p, 12345, np.arange(N_DRAWS))
    counts = np.bincount(o.token, minlength=64)
    assert counts[q == 0].sum() == 0, "a token outside the support"
    assert np.isfinite(x[o.token]).all()
    if kind == "ties":  # a filter that cuts a group of equal logits keeps the whole group
        sup = q > 0
        assert all(sup[x == v].all() or not sup[x == v].any() for v in np.unique(x))
    if k > 0 or p < 1:
        assert 2 <= (q > 0).sum() < np.isfinite(x).sum() and o.rounds.max() >= 2
    keep = q * N_DRAWS >= 5  # the usual validity rule of the chi-square test; the rest pooled
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(q[keep], q[~keep].sum()) * N_DRAWS
    obs, exp = obs[exp > 0], exp[exp > 0]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    limit = _chi2_quantile(0.999, len(obs) - 1)
    print(f"{kind} T={T} k={k} p={p}: chi2 {chi2:.1f} < {limit:.1f} ({len(obs) - 1} dof), "
          f"ambiguous {o.ambiguous.mean():.4%}")
    assert chi2 < limit


def _chi2_quantile(prob: float, dof: int) -> float:
    """x with P(chi2_dof <= x) = prob: bisection on the regularised lower incomplete gamma function."""
    a = torch.tensor(dof / 2, dtype=torch.float64)
    lo, hi = 0.0, 10.0 * dof + 100.0
    for _ in range(80):
        mid = (lo + hi) / 2
        if float(torch.special.gammainc(a, torch.tensor(mid / 2, dtype=torch.float64))) < prob:
            lo = mid
        else:
            hi = mid
    return hi


def test_chi2_quantile_matches_the_tables():
    for dof, want in ((1, 10.828), (9, 27.877), (10, 29.588), (50, 86.661), (63, 103.442)):
        assert abs(_chi2_quantile(0.999, dof) - want) < 2e-3


def _sample_ref_keep(row, t, k, p):
    """The set vgate.ops.reference.sample_ref keeps (its filter, line by line)."""
    probs = torch.softmax(row.float() / t, dim=-1)
    sp, si = torch.sort(probs, descending=True)
    keep = torch.ones_like(sp, dtype=torch.bool)
    if 0 < k < row.numel():
        keep[k:] = False
    if p < 1.0:
        csum = torch.cumsum(sp, 0)
        keep &= (csum - sp) < p
    out = torch.zeros(row.numel(), dtype=torch.bool)
    out[si[keep]] = True
    return out.numpy()


@pytest.mark.parametrize("T,k,p", [(1.0, -1, 1.0), (0.7, 5, 1.0), (1.0, -1, 0.8), (1.5, 40, 0.95), (0.3, 300, 0.5),
                                   (1.0, 1, 1.0), (1.0, 999, 1.0), (1.0, 1000, 0.999)])
def test_support_equals_what_sample_ref_keeps(T, k, p):
    g = torch.Generator().manual_seed(21)
    row = torch.randn(1000, generator=g) * 2
    assert len(torch.unique(row)) == 1000  # no ties: both definitions agree
    sup = sc.support(row.numpy(), T, k, p)
    assert np.array_equal(sup, _sample_ref_keep(row, T, k, p))
    gens = [torch.Generator().manual_seed(3)]
    for _ in range(20):  # and sample_ref itself stays inside it
        t = int(ref.sample_ref(row[None], torch.tensor([T]), torch.tensor([p]), torch.tensor([k]), gens)[0])
        assert sup[t]
    for off in range(20):
        assert sup[sc.oracle_row(row.numpy(), T, k, p, 8, off)[0]]


# ------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_ambiguous_share_is_within_the_cap(name):
    """Exact cases have no ambiguous row; every other case at most 1 % (a case above the cap gets
    another seed, the cap stays). Every token lies in the row's support."""
    c = sc.build_case(name)
    kind = sc.CASES[name][0]
    share = float(c.ambiguous.mean())
    finite = c.gap_ratio[np.isfinite(c.gap_ratio)]
    print(f"{name}: ambiguous {int(c.ambiguous.sum())}/{c.ambiguous.size} = {share:.2%}, max rounds "
          f"{int(c.rounds.max())}, min key gap / tau {finite.min() if finite.size else float('inf'):.3g}")
    assert c.exact == (kind in sc.EXACT_KINDS)
    assert share == 0.0 if c.exact else share <= 0.01
    assert c.nseg == sc.segments(c.B, c.V) and c.ldl == c.V + sc.PAD
    assert bool((c.buf[:, c.V:] == sc.GUARD).all())
    x, T = c.x, c.temperature.numpy()
    for b in range(min(c.B, 16)):
        if T[b] > np.float32(1e-5):
            sup = sc.support(x[b], T[b], int(c.top_k[b]), float(c.top_p[b]), slack=True)
            assert sup[c.token[:, b]].all(), (name, b)
        else:
            assert (c.token[:, b] == int(np.argmax(x[b]))).all()
    if kind.startswith("chain"):
        assert c.rounds.max() >= 8  # the chains stay deep
    if kind in ("chain_k1", "topp0"):
        assert np.array_equal(c.token, np.broadcast_to(np.argmax(x, axis=1), c.token.shape))
    if kind == "masked":
        m = sc.masked_rows(c.B)  # exact rows: token 0 without a draw, never ambiguous
        assert (c.token[:, m] == 0).all() and (c.rounds[:, m] == 0).all() and not c.ambiguous[:, m].any()
    if kind in ("equal", "strided"):
        for o in range(c.offsets.shape[0]):
            u = sc.uniforms(c.seeds.numpy(), c.offsets[o].numpy(), c.V, 0)
            assert np.array_equal(c.token[o], np.argmax(np.where(np.isfinite(x), u, 0.0), axis=1))
    if kind == "ties":
        for b in range(min(c.B, 8)):  # top_k falls inside a group of equal logits
            k = int(c.top_k[b])
            if k > 0:
                xs = np.sort(x[b])[::-1]
                assert xs[k - 1] == xs[k]
                assert sc.support(x[b], T[b], k, 1.0)[x[b] == xs[k]].all()  # and the whole group stays
            if float(c.top_p[b]) < 1:  # top_p ends inside a group: all of it in, the next value out
                sup = sc.support(x[b], T[b], -1, float(c.top_p[b]))
                last = x[b][sup].min()
                assert (x[b] == last).sum() >= 2 and sup[x[b] == last].all() and not sup[x[b] < last].any()
