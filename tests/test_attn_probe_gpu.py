"""Closed-form per-row probes of the attention kernels (tests/attn_probe.py; the probes themselves are
proved on the CPU by tests/test_attn_probe_cpu.py): every element of every output row of every launch
is compared with an expectation that needs no softmax code, at the mask, page, chunk, partition and
K-split edges of the decode block, the partition reduce kernel, the 16-query tile kernel and the
flash prefill kernel. A failure prints which cache row the kernel returned in place of the expected one.

Run on an MI355X: ``python -m pytest tests/test_attn_probe_gpu.py -m gpu`` (``-s`` prints the rows
checked per path and the largest observed error as a fraction of the tolerance)."""
import functools

import pytest
import torch

import attn_probe as ap
import gemm_exact as X
from vgate import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ap.D


@pytest.fixture(autouse=True, scope="module")
def _native():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ops.native()  # must load: no silent fallback
    yield
    for path, st in sorted(ap.STATS.items()):
        print(f"\nattn probes [{path}]: {st['rows']} rows, largest |out - expected| / tolerance: "
              f"one-hot {st['onehot']:.4f}, uniform {st['uniform']:.4f}", end="")
    print()


class Dev:
    """A case on the device: cache, tables, the queries of every round (plain rows and inside a fused
    qkv row whose k / v columns hold poison), each allocated at its exact size, and the partition buffers."""

    def __init__(self, sp: ap.Spec):
        c = self.case = ap.build(sp)
        self.kc, self.vc = c.kc.to(DEV), c.vc.to(DEV)
        self.kc0, self.vc0 = self.kc.clone(), self.vc.clone()
        self.bt, self.cl, self.qs = c.bt.to(DEV), c.cl.to(DEV), c.qs.to(DEV)
        self.wide = (sp.Hq + 2 * sp.Hkv) * D
        q = torch.full((c.R, c.T, self.wide), ap.POISON_V, dtype=torch.bfloat16)
        q[:, :, : sp.Hq * D] = c.q
        self.q_wide = q.to(DEV)
        self.q = self.q_wide[:, :, : sp.Hq * D].contiguous()
        self.P = (c.maxb * ap.BS + sp.part - 1) // sp.part if sp.part else 1
        self.po = torch.full((c.S, sp.Hq, self.P, D), float("nan"), device=DEV)
        self.pml = torch.full((c.S, sp.Hq, self.P, 2), float("nan"), device=DEV)
        self.empty = torch.empty(0, dtype=torch.int32, device=DEV)

    def out_buffer(self):
        """[R, GUARD + T + GUARD, Hq * D] of the sentinel; round r's launch writes view(r)."""
        c = self.case
        return torch.full((c.R, c.T + 2 * ap.GUARD, c.spec.Hq * D), ap.SENT, dtype=torch.bfloat16, device=DEV)

    def view(self, buf, r):
        return buf[r, ap.GUARD: ap.GUARD + self.case.T]

    def caches_untouched(self, what=""):
        """After every launch: attention must not write K or V."""
        assert torch.equal(self.kc, self.kc0) and torch.equal(self.vc, self.vc0), f"attention wrote the KV cache: {what}"


def _has_flash(Hq, Hkv) -> bool:
    """attention.hip flash_cfg: 8 waves when G divides 8, 6 when it divides 6, else the tile kernel.
    (The same head-group rule as flash_cfg and ops.flash_lead: change the three together.)"""
    G = Hq // Hkv
    return 8 % G == 0 or 6 % G == 0


def _flash_zs(ents, tiles: int, dec_rows: int, Hkv: int):
    """From the launch timeline: None when the 16-query tile kernel ran (flash off, or a head group
    flash_cfg declines), else the K-split factor zs of the flash launch, whose grid is
    (tiles + decode rows) x Hkv x zs blocks."""
    fl = [e for e in ents if e[0] == "attn_flash"]
    if not fl:
        assert any(e[0] == "attention" for e in ents), ents
        return None
    assert len(fl) == 1 and fl[0][2] % ((tiles + dec_rows) * Hkv) == 0, (fl, tiles, dec_rows, Hkv)
    return fl[0][2] // ((tiles + dec_rows) * Hkv)


@functools.lru_cache(maxsize=4)
def dev(sp: ap.Spec) -> Dev:
    return Dev(sp)


def _tiles(qlens, Hq, Hkv, order: str, seed: int = 0):
    """The engine's tile list plus 5 padding tiles of a graph bucket; "shuffled": the same list in a
    seeded random order (correctness does not depend on the order, ops.tile_order)."""
    ts, tq = ops.prefill_tiles(list(qlens), ops.flash_lead(Hq, Hkv))
    ts, tq = ts + [-1] * 5, tq + [0] * 5
    if order == "shuffled":
        g = torch.Generator()
        g.manual_seed(77 + seed)
        perm = torch.randperm(len(ts), generator=g).tolist()
        ts, tq = [ts[i] for i in perm], [tq[i] for i in perm]
    return (torch.tensor(ts, dtype=torch.int32, device=DEV), torch.tensor(tq, dtype=torch.int32, device=DEV))


def _decode_ticket(d: Dev, r: int, out):
    """Decode rows through the unified launch without tiles: partitions merged in-launch by the last
    arriving block (tickets: the per-device default)."""
    sp = d.case.spec
    ops.attention(d.q[r], sp.Hq * D, d.kc, d.vc, d.bt, d.cl, d.qs, d.empty, d.empty, out, d.po, d.pml, sp.Hq, sp.Hkv,
                  sp.part, ap.SCALE)


def _decode_reduce(d: Dev, r: int, out, query_start=None):
    """attn_decode: partials to part_o / part_ml, merged by attn_decode_reduce_kernel."""
    sp = d.case.spec
    ops.attention_decode(d.q[r], sp.Hq * D, d.kc, d.vc, d.bt, d.cl, out, d.po, d.pml, sp.Hq, sp.Hkv, sp.part, ap.SCALE,
                         query_start=query_start)


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("part", ap.PARTS)
@pytest.mark.parametrize("Hq,Hkv", ap.LAYOUTS)
def test_decode_probes(Hq, Hkv, part, group):
    """Contexts 1 .. 1025 around every page, chunk and partition edge (one chunk per wave, more chunks
    than waves, 1 / 2 / 17 partitions, last partitions of one token), every round of queries, through
    the in-launch ticket merge and through the partials + reduce kernel. The two merges divide
    differently (x * (1 / L) against x / L), so each is held to the closed form, not to the other."""
    d = dev(ap.decode_spec(Hq, Hkv, part, group))
    c = d.case
    for path, run in (("decode, ticket merge", _decode_ticket), ("decode, reduce kernel", _decode_reduce)):
        buf = d.out_buffer()
        for r in range(c.R):
            run(d, r, d.view(buf, r))
            d.caches_untouched(f"{path}, round {r}")
        ap.check(c, buf, path)


@pytest.mark.parametrize("Hq,Hkv", ap.LAYOUTS)
def test_decode_repeated_on_the_same_buffers(Hq, Hkv):
    """One launch three times over the same output, partials and tickets (the tickets re-arm themselves;
    the conftest checks the words after the test)."""
    d = dev(ap.decode_spec(Hq, Hkv, 64, 1))
    buf = d.out_buffer()
    for rep in range(3):
        for r in range(d.case.R):
            _decode_ticket(d, r, d.view(buf, r))
            d.caches_untouched(f"repeat {rep}, round {r}")
    ap.check(d.case, buf, "decode, ticket merge")


@pytest.mark.parametrize("Hq,Hkv", ap.LAYOUTS)
def test_decode_query_start(Hq, Hkv):
    """Decode rows at query_start[s + 1] - 1 of a wider q: sequences of 0, 2 and 3 queries are not
    decode work, their rows keep the sentinel. The last sequence is empty: its query_start is the row
    behind q, which a decode block must not read (it used to fetch the query before testing the length)."""
    d = dev(ap.query_start_spec(Hq, Hkv, 64))
    buf = d.out_buffer()
    for r in range(d.case.R):
        _decode_reduce(d, r, d.view(buf, r), query_start=d.qs)
        d.caches_untouched(f"round {r}")
    ap.check(d.case, buf, "decode, reduce kernel", decode_only=True)


@pytest.mark.parametrize("order", ["engine", "shuffled"])
@pytest.mark.parametrize("variant", ["flash_split", "flash", "tile"])
@pytest.mark.parametrize("Hq,Hkv", ap.LAYOUTS)
def test_prefill_probes(Hq, Hkv, variant, order):
    """Whole and chunked prefills (cached prefixes 0 / 36-37 / 237 / 260, ragged last tiles, ranges of
    >= 4 flash chunks) with q read from inside a fused qkv row, on the flash kernel with and without the
    K split and on the 16-query tile kernel, tile list in the engine's order and shuffled."""
    C = ops.native()
    d = dev(ap.prefill_spec(Hq, Hkv))
    c = d.case
    ts, tq = _tiles(c.spec.qlens, Hq, Hkv, order)
    buf = d.out_buffer()
    zs = set()
    try:
        C.set_flash_prefill(0 if variant == "tile" else 1)
        ops.FLASH_SPLIT = variant == "flash_split"
        for r in range(c.R):
            ents = X.launches(lambda: ops.attention_prefill(d.q_wide[r], d.wide, d.kc, d.vc, d.bt, d.cl, d.qs, ts, tq,
                                                            d.view(buf, r), Hq, Hkv, ap.SCALE))
            zs.add(_flash_zs(ents, ts.numel(), 0, Hkv))
            d.caches_untouched(f"round {r}")
    finally:
        ops.FLASH_SPLIT = True
        C.set_flash_prefill(-1)
    # the kernel that ran, from the timeline: G = 5 has no flash configuration and keeps the tile kernel
    declined = not _has_flash(Hq, Hkv)
    if variant == "tile" or declined:
        assert zs == {None}, zs
        path = "prefill, tile kernel"
    elif variant == "flash":
        assert zs == {1}, zs
        path = "prefill, flash"
    else:  # the ranges of >= 4 chunks (contexts 300 and 330) ran as min(zs, chunks / 2) parts
        assert zs <= {2, 4} and zs, zs
        path = "prefill, flash K split"
    ap.check(c, buf, path)


@pytest.mark.parametrize("flash", [1, 0])
@pytest.mark.parametrize("part", ap.MIXED_PARTS)
@pytest.mark.parametrize("Hq,Hkv", ap.LAYOUTS)
def test_mixed_step_probes(Hq, Hkv, part, flash):
    """The unified launch: the prefill list with single-query sequences of context 5, 64, 65 and 700 in
    between (decode blocks, partitions merged in-launch). With part 64 the tile list names every
    sequence (the kernels leave a single-query sequence's tile to the decode block), with 512 only
    the prefill sequences. The step ends with two empty sequences, as a padded graph bucket does: their
    query_start is the row behind q, and every decode block of theirs runs."""
    C = ops.native()
    d = dev(ap.mixed_spec(Hq, Hkv, part))
    c = d.case
    qlens = c.spec.qlens if part == 64 else [ql if ql > 1 else 0 for ql in c.spec.qlens]
    ts, tq = _tiles(qlens, Hq, Hkv, "engine")
    buf = d.out_buffer()
    zs = set()
    try:
        C.set_flash_prefill(flash)
        for r in range(c.R):
            ents = X.launches(lambda: ops.attention(d.q[r], Hq * D, d.kc, d.vc, d.bt, d.cl, d.qs, ts, tq, d.view(buf, r),
                                                    d.po, d.pml, Hq, Hkv, part, ap.SCALE))
            zs.add(_flash_zs(ents, ts.numel(), c.S * d.P, Hkv))
            d.caches_untouched(f"round {r}")
    finally:
        C.set_flash_prefill(-1)
    declined = not _has_flash(Hq, Hkv)
    if not flash or declined:
        assert zs == {None}, zs
        path = "mixed step, tile kernel"
    else:  # (ops.FLASH_SPLIT is on: the K split runs here too)
        assert zs <= {2, 4} and zs, zs
        path = "mixed step, flash K split"
    ap.check(c, buf, path)
