"""The sampler on the MI355X: csrc/kernels/sampling.hip (sample_gran_kernel and sample_row_kernel)
against the float64 per-draw oracle of tests/sampler_cases.py. Every row whose decisions fp32 can
resolve must return the oracle's token exactly; the others (printed share, capped at 1 % per case
by tests/test_sampler_cpu.py) must stay inside the oracle's support.

out_logprob is the tempered, unfiltered log-softmax at the chosen id,
((x - mx) c - log2 z) / log2e with c = log2e / T. Bound |got - ref| <= (V/256 + 64) 2^-24 +
2^-22 |ref| + 1e-6: z is a sum of up to V/256 sequential terms per thread plus merges (the mass band
of sampler_cases), relative in z and so absolute in ln z; the product and the two roundings of the
difference are relative to |x - mx| / T and ln z, both at most |ref|; log2f and the division 1e-6.
"""
import numpy as np
import pytest
import torch

import sampler_cases as sc
from vgate import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch(c, buf, par, o, **kw):
    T, tk, tp, seeds = par
    return ops.sample(buf[:, : c.V], T, top_p=tp, top_k=tk, seeds=seeds, offsets=c.offsets[o].to(DEV), **kw)


def _params(c):
    return c.temperature.to(DEV), c.top_k.to(DEV), c.top_p.to(DEV), c.seeds.to(DEV)


def _check_ids(c, o, ids, what):
    """Unambiguous rows equal the oracle; ambiguous rows lie in its support."""
    ids = ids.cpu().numpy().astype(np.int64)
    amb = c.ambiguous[o]
    bad = np.nonzero((ids != c.token[o]) & ~amb)[0]
    assert bad.size == 0, (what, [(int(b), int(ids[b]), int(c.token[o][b]), int(c.rounds[o][b])) for b in bad[:8]])
    for b in np.nonzero(amb)[0]:
        sup = sc.support(c.x[b], float(c.temperature[b]), int(c.top_k[b]), float(c.top_p[b]), slack=True)
        assert 0 <= ids[b] < c.V and sup[ids[b]], (what, int(b), int(ids[b]))
    return ids


@pytest.mark.parametrize("name", list(sc.CASES))
def test_kernels_equal_the_oracle(name):
    c = sc.build_case(name)
    kind = sc.CASES[name][0]
    C = ops.native()
    buf, par = c.buf.to(DEV), _params(c)
    fault0 = ops.fault_word(DEV).clone()
    want_lp = kind == "logprob"
    worst = 0.0
    try:
        for cap in (64,) + sc.NSEG_CAPS:  # the default first; uneven v_lo / v_hi at 7 and 33
            C.set_sample_nseg(cap)
            nseg = sc.segments(c.B, c.V, cap)
            assert C.sample_segments(c.B, c.V) == nseg and (cap != 64 or nseg == c.nseg)
            for o in range(c.offsets.shape[0]):
                what = f"{name} nseg={nseg} launch={o}"
                lp = torch.full((c.B,), float("nan"), device=DEV) if want_lp else None
                ids = _launch(c, buf, par, o, out_logprob=lp).clone()
                again = _launch(c, buf, par, o)
                assert torch.equal(ids, again), what  # reproducible for a (seed, offset)
                got = _check_ids(c, o, ids, what)
                if kind in ("chain_k1", "topp0"):  # the argmax whatever the path
                    assert np.array_equal(got, np.argmax(c.x, axis=1)), what
                if kind == "masked":
                    assert (got[sc.masked_rows(c.B)] == 0).all(), what
                if want_lp:
                    ref = sc.logprob_ref(c.x, c.temperature.numpy(), got)
                    err = np.abs(lp.cpu().numpy().astype(np.float64) - ref)
                    bound = (c.V / 256 + 64) * 2.0 ** -24 + 2.0 ** -22 * np.abs(ref) + 1e-6
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (what, float((err / bound).max()))
    finally:
        C.set_sample_nseg(64)
    torch.cuda.synchronize()
    assert torch.equal(ops.fault_word(DEV), fault0)
    assert bool((buf[:, c.V:] == sc.GUARD).all())
    print(f"{name}: skipped (ambiguous) {int(c.ambiguous.sum())}/{c.ambiguous.size} = {c.ambiguous.mean():.2%}"
          + (f", logprob max |err| / bound = {worst:.3f}" if want_lp else ""))


@pytest.mark.parametrize("name", ["general-8196x130", "ties-8196x130", "general-151936x8"])
def test_a_row_draws_the_same_token_at_any_batch_position_and_size(name):
    """A row's token depends on its logits, parameters, seed and offset alone: rows 4..6 launched as
    a batch of 3 (another segment count, or the other kernel), and copies of row 4 at other positions
    of the full batch."""
    c = sc.build_case(name)
    buf, (T, tk, tp, seeds) = c.buf.to(DEV), _params(c)
    offs = c.offsets[0].to(DEV)
    full = ops.sample(buf[:, : c.V], T, top_p=tp, top_k=tk, seeds=seeds, offsets=offs).clone()
    s = slice(4, 7)
    assert ops.native().sample_segments(3, c.V) != ops.native().sample_segments(c.B, c.V)
    sub = ops.sample(buf[s, : c.V], T[s], top_p=tp[s], top_k=tk[s], seeds=seeds[s], offsets=offs[s])
    assert torch.equal(sub, full[s])
    for t in (buf, T, tk, tp, seeds, offs):
        t[1] = t[4]
        t[c.B - 1] = t[4]
    twins = ops.sample(buf[:, : c.V], T, top_p=tp, top_k=tk, seeds=seeds, offsets=offs)
    assert int(twins[1]) == int(twins[c.B - 1]) == int(full[4])
    keep = [b for b in range(c.B) if b not in (1, c.B - 1)]
    assert torch.equal(twins[keep], full[keep])
