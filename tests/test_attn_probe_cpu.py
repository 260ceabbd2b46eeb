"""The attention probes of tests/attn_probe.py proved without a GPU: for every case the GPU file
launches, the closed-form expectation is reproduced by two independent softmax references, the
needle keys keep their logit gap, and ten deliberately wrong kernels (mutants of the float64
reference) are all caught by the very check function the GPU tests use, with a diagnosis that names
the position the wrong kernel returned."""
import math
import re

import pytest
import torch

import attn_probe as ap
from vgate.ops import reference as ref

SPECS = ap.all_specs()
IDS = [ap.spec_id(sp) for sp in SPECS]


def _rel_err(a, b):  # the statistic of the attention tests in tests/test_kernels_gpu.py
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


@pytest.mark.parametrize("sp", SPECS, ids=IDS)
def test_preconditions(sp):
    c = ap.build(sp)
    # every operand is a bf16 value (bf16_exact asserted it on the way in), the poison is finite and
    # every table entry names a block of the cache
    for t in (c.q, c.kc, c.vc):
        assert t.dtype == torch.bfloat16 and bool(torch.isfinite(t.float()).all())
    assert int(c.bt.min()) >= 0 and int(c.bt.max()) < c.nblk
    assert bool((c.bt == 0).any()), "block 0 is some sequence's page"
    named = set(c.bt.flatten().tolist())
    assert len(named) < c.nblk and c.poison_blk in named, "unnamed poison blocks and a named one"
    for s in range(c.S):
        pages = c.bt[s, : c.npg[s]].tolist()
        assert c.npg[s] < 3 or any(b - a != 1 for a, b in zip(pages, pages[1:])), "pages are not contiguous"
        assert set(c.bt[s, c.npg[s]:].tolist()) <= {c.poison_blk}
    assert ap.needle_gaps(c) >= ap.NEEDLE_GAP
    live = c.live
    kinds = c.kind[:, live]
    for kd in range(4):
        assert bool((kinds == kd).any()), ap.KINDS[kd]
    # needles at qpos, at ctx - qlen, at a page edge, a 32-edge and a 64-edge (where the case has one)
    nd = (c.kind == ap.NEEDLE) & live[None, :, None]
    tg = c.target[nd]
    qpos = c.qpos[None, :, None].expand_as(c.kind)[nd]
    first = torch.tensor([sp.ctxs[s] - sp.qlens[s] for s in c.tok_seq.tolist()])[None, :, None].expand_as(c.kind)[nd]
    assert bool((tg == qpos).any()) and bool((tg == first).any())
    top = int(c.qpos[live].max())
    for lo, hi in ((15, 16), (31, 32), (63, 64)):
        if top >= hi:
            assert bool(((tg == lo) | (tg == hi)).any()), (lo, hi)
    if sp.rounds == ap.DECODE_ROUNDS and top >= sp.part:  # the decode cases: a needle at a partition edge
        assert bool(((tg == sp.part - 1) | (tg == sp.part)).any()), "partition edge"


@pytest.mark.parametrize("sp", SPECS, ids=IDS)
def test_references_reproduce_the_closed_form(sp):
    c = ap.build(sp)
    # 1. float64, per row, explicit visible set: within 0.01 of every expectation
    buf = ap.ref64(c)
    out = buf[:, ap.GUARD:ap.GUARD + c.T].reshape(c.R, c.T, sp.Hq, ap.D)
    assert float((out[:, c.live] - c.expected[:, c.live]).abs().max()) <= 0.01
    res = ap.check(c, buf)
    assert res["rows"] == c.R * int(c.live.sum()) * sp.Hq
    # 2. the project's fp32 oracle (bf16 output): within the GPU tolerances
    buf2 = torch.full_like(buf, ap.SENT)
    for r in range(c.R):
        o = ref.attention_ref(c.q[r].view(c.T, sp.Hq, ap.D), c.kc, c.vc, c.bt, c.cl, c.qs, sp.Hq, sp.Hkv, ap.SCALE)
        o = o.reshape(c.T, -1).double()
        buf2[r, ap.GUARD:ap.GUARD + c.T][c.live] = o[c.live]
    ap.check(c, buf2)


# what the diagnosis of each mutant must say (the right position, or what was read in its place)
def _expected_diagnosis(c, mutate):
    sp = c.spec
    if mutate == "causal+1":
        return r"kind latest: expected position (\d+), got position (\d+) of seq", lambda m: int(m[2]) == int(m[1]) + 1
    if mutate == "causal-1":
        return (r"kind latest: expected position (\d+), got (?:position (\d+) of seq|zeros)",
                lambda m: int(m[1]) == 0 if m[2] is None else int(m[2]) == int(m[1]) - 1)
    if mutate == "ctx+1":  # one key past the bound: the next query's key, or the stale slot's poison
        return (r"kind latest: expected position (\d+), got (?:position (\d+) of seq|poison 240)",
                lambda m: m[2] is None or int(m[2]) == int(m[1]) + 1)
    if mutate == "drop0":
        return r"kind earliest: expected position 0, got (?:position 1 of seq|zeros)", None
    if mutate == "chunk32":
        return r"kind needle: expected position (31|32), got ", None
    if mutate == "partition":
        return r"kind (?:needle|latest): expected position (\d+), got ", lambda m: int(m[1]) >= sp.part
    if mutate == "table":
        return r"kind earliest: expected position 0, got position 16 of seq", None
    if mutate == "kvhead":
        return r"head 0 kind \w+: expected .*kv head 1", None
    if mutate == "swap":
        return r"seq (\d+) token .* got .*of seq (\d+)", lambda m: m[1] != m[2]
    if mutate == "rowlate":
        return r"got the untouched sentinel", None
    raise AssertionError(mutate)


# only the pairs whose mutated edge exists in the case (a decode-only case has no causal bound above
# the context, a single KV head no neighbour, ...)
MUTANT_PAIRS = [(sp, m) for sp in SPECS for m in ap.MUTANTS if ap.mutant_exists(sp, m)]


def test_every_mutant_meets_every_kind_of_case():
    for m in ap.MUTANTS:
        assert {sp.name for sp, mm in MUTANT_PAIRS if mm == m} >= ({"mixed"} if m == "causal+1" else {"decode", "mixed"}), m
    assert {sp.name for sp, mm in MUTANT_PAIRS if mm == "causal+1"} >= {"prefill", "mixed", "qstart"}


@pytest.mark.parametrize("sp,mutate", MUTANT_PAIRS, ids=[f"{ap.spec_id(sp)}-{m}" for sp, m in MUTANT_PAIRS])
def test_mutants_are_caught(sp, mutate):
    c = ap.build(sp)
    with pytest.raises(AssertionError) as ei:
        ap.check(c, ap.ref64(c, mutate))
    msg = str(ei.value)
    pat, ok = _expected_diagnosis(c, mutate)
    hits = [m for m in re.finditer(pat, msg)]
    assert hits and (ok is None or any(ok(m) for m in hits)), msg


def test_guards_dead_rows_and_nan_are_caught():
    c = ap.build(ap.query_start_spec(12, 2, 64))
    good = ap.ref64(c)
    decode_rows = good.clone()
    decode_rows[:, ap.GUARD:ap.GUARD + c.T][:, ~c.live_decode] = ap.SENT
    ap.check(c, decode_rows, decode_only=True)
    with pytest.raises(AssertionError, match="no work in this launch"):
        ap.check(c, good, decode_only=True)  # the rows of the 2- and 3-query sequences were written
    for row, name in ((ap.GUARD - 1, "guard row -1"), (ap.GUARD + c.T, f"guard row {c.T}")):
        bad = good.clone()
        bad[0, row, 5] = 1.0
        with pytest.raises(AssertionError, match=name):
            ap.check(c, bad)
    bad = good.clone()
    bad[1, ap.GUARD, 3] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        ap.check(c, bad)
    bad = good.clone()  # one element of one row, off by just over the one-hot tolerance
    r, t, hq = [int(x) for x in (c.kind[:, c.live] == ap.LATEST).nonzero()[0]]
    t = int(c.live.nonzero().flatten()[t])
    bad[r, ap.GUARD + t, hq * ap.D + 77] += 1.5
    with pytest.raises(AssertionError, match="1 of"):
        ap.check(c, bad)


def test_norm_statistic_misses_what_the_probes_catch():
    """Why this file exists: on the randn inputs of test_attention_decode (contexts [513, 2048, 1500,
    64]) a kernel that reads one stale slot past the context, or drops the last key, of the two long
    sequences stays under that test's gate, rel. error < 2e-2."""
    torch.manual_seed(6)
    Hq, Hkv, ctxs = 12, 2, [513, 2048, 1500, 64]
    S, maxb = len(ctxs), 2048 // 16 + 1
    nblk = S * maxb + 8
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = torch.randn(nblk, Hkv, 16, 128, generator=g).bfloat16()
    vc = torch.randn(nblk, Hkv, 16, 128, generator=g).bfloat16()
    bt = (torch.randperm(nblk - 1)[: S * maxb] + 1).reshape(S, maxb).int()
    cl = torch.tensor(ctxs, dtype=torch.int32)
    qs = torch.arange(S + 1, dtype=torch.int32)
    q = torch.randn(S, Hq * 128).bfloat16()
    scale = 1 / math.sqrt(128)
    args = (q, kc, vc, bt, cl, qs, Hq, Hkv, scale)
    good = ap.attention64(*args)
    fp32 = ref.attention_ref(q.view(S, Hq, 128), kc, vc, bt, cl, qs, Hq, Hkv, scale)
    assert _rel_err(fp32[None], good) < 5e-3  # the two references agree to bf16 output rounding
    for mutate in ("ctx+1", "causal-1"):
        wrong = ap.attention64(*args, mutate=mutate, seqs={1, 2})
        assert not torch.equal(wrong[0, 1], good[0, 1]) and not torch.equal(wrong[0, 2], good[0, 2])
        assert torch.equal(wrong[0, 0], good[0, 0]) and torch.equal(wrong[0, 3], good[0, 3])
        assert _rel_err(wrong, good) < 2e-2, mutate
