"""Logprobs on the MI355X: csrc/kernels/logprobs.hip against the float64 oracle (ids exact, values
within a derived bound), and the engine with logprobs requests across capture and scheduling modes.

The value bound |got - ref| <= 1e-5 + 2^-22 |ref|, from the kernels' reduction shape:
  got = (x - m) - ln(l), l = sum 2^((x_i - m) log2e) accumulated as
    * per thread: 20 adds per chunk of 5 float4, then one merge (exp2 of the max difference, product,
      add) per further chunk: 1 chunk at 32 segments, 30 chunks at V = 151936 with one block per row;
    * per wave: one rescale to the wave maximum (exp2, product) and a 6-level add tree;
    * per block: 3 merges of the waves; per row: one rescale per segment and 31 adds in segment order.
  A plain add costs 0.5 ulp, a rescale 2 ulp, a merge 2.5 ulp, and each term carries at most 2 ulp of
  its own (exp2 and its rounded argument, weighted by the term). One block per row:
  2 + 20 * 0.5 + 29 * 2.5 + 2 + 6 * 0.5 + 3 * 2.5 + 2 = 99 ulp; 32 segments: 2 + 10 + 2 + 3 + 7.5 + 2 +
  31 * 0.5 = 42 ulp. 99 ulp = 5.9e-6 relative in l, an absolute 5.9e-6 in ln(l) in the worst case
  (errors of random sign stay near the square root of that). ln adds 1 ulp at |ln l| <= 12 (1e-6);
  the two subtractions round at |x - m| and |got|, each at most 2^-24 of a magnitude that |ref|
  bounds up to ln(l): covered by 2^-22 |ref|. Sum of the absolute parts: 6.9e-6 < 1e-5.
"""
import pytest
import torch

from logprobs_cases import GUARD, build_case, check_entries, segments
from vgate import ops
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77


def _check_values(got, want, what):
    """got fp32, want float64: -inf exactly, finite entries within the module docstring's bound."""
    got = got.double()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got) & (got < 0), inf), what
    err = (got - want).abs()[~inf]
    bound = (1e-5 + 2.0 ** -22 * want.abs())[~inf]
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"{what}: max |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("V", [20, 21, 1000, 4099, 151936])
@pytest.mark.parametrize("S", [1, 3, 8, 130])
def test_kernels_equal_the_oracle(S, V):
    c = build_case(V, S)
    assert ops.native().logprob_segments(S, V) == segments(S, V)
    buf = c.buf.to(DEV)
    lg = buf[:, :V]  # row stride above V, the padding columns hold 1e30
    tokens, k_rows = c.tokens.to(DEV), c.k_rows.to(DEV)
    fault0 = ops.fault_word(DEV).clone()
    out = torch.full((S, ops.LOGPROB_REC_WORDS), SENTINEL, dtype=torch.int32, device=DEV)
    chosen, top_ids, top_lp = ops.logprobs(lg, tokens, k_rows, out=out)
    again = torch.full_like(out, SENTINEL)
    ops.logprobs(lg, tokens, k_rows, out=again)
    torch.cuda.synchronize()
    assert torch.equal(out, again)  # bit-reproducible
    assert torch.equal(ops.fault_word(DEV), fault0)
    assert bool((buf[:, V:] == GUARD).all())
    asked = c.k_rows >= 0
    rec = out.cpu()
    assert bool((rec[~asked] == SENTINEL).all())  # rows that did not ask are left untouched
    assert torch.equal(rec[asked, 0].long(), c.tokens[asked].long().clamp(0, V - 1))
    assert bool((rec[asked, 42:] == 0).all())
    assert torch.equal(top_ids.cpu()[asked].long(), c.top_ids[asked]), \
        [r for r in range(S) if asked[r] and not torch.equal(top_ids[r].cpu().long(), c.top_ids[r])]
    _check_values(chosen.cpu()[asked], c.chosen[asked], f"chosen V={V} S={S}")
    _check_values(top_lp.cpu()[asked], c.top_lp[asked], f"top V={V} S={S}")


# ------------------------------------------------------------------------------------- engine
PROMPTS = {f"q{i}": [3 + (i * 31 + j * 17) % 500 for j in range(7 + 9 * i)] for i in range(3)}
X = 77


def _engine(**kw):
    cfg = dict(model="tiny", device="cuda", max_model_len=512, max_num_seqs=16, max_num_batched_tokens=256,
               num_kv_blocks=256, warmup=False, seed=0)
    cfg.update(kw)
    eng = LLMEngine(EngineConfig(**cfg))
    eng.runner.defer_capture = False
    return eng


def _run(eng, lp: bool):
    """One batch: a logprobs request, a plain request and a logit_bias request that also sets logprobs
    (``lp`` False: the same three without logprobs)."""
    g = dict(temperature=0.0, ignore_eos=True, max_tokens=12)
    sps = [SamplingParams(logprobs=5 if lp else None, **g), SamplingParams(**g),
           SamplingParams(logprobs=2 if lp else None, logit_bias={X: 100.0}, **g)]
    done = {}
    for (rid, ids), sp in zip(PROMPTS.items(), sps):
        eng.add_request(rid, params=sp, prompt_ids=ids, callback=lambda k, s, p: done.update({s.request_id: s}))
    eng.run_until_idle()
    return done


@pytest.fixture(scope="module")
def graph_runs():
    with_lp, without = _engine(), _engine()
    assert with_lp.async_sched and with_lp.runner.use_graphs
    return with_lp, _run(with_lp, True), without, _run(without, False)


def test_engine_mixed_batch_with_graphs(graph_runs):
    eng, a, base, b = graph_runs
    for k in PROMPTS:
        assert a[k].output_ids == b[k].output_ids and len(a[k].output_ids) == 12, k
    check_entries(a["q0"], 5)
    assert a["q1"].logprobs is None and all(s.logprobs is None for s in b.values())
    assert a["q2"].output_ids == [X] * 12
    for tid, lp, top in a["q2"].logprobs:  # the distribution after the processors
        assert tid == X and lp > -1e-3 and len(top) == 2 and top[0] == (X, lp)
    r, r0 = eng.runner, base.runner
    assert r.lp_steps > 0 and eng.snapshot()["lp_steps"] == r.lp_steps
    assert r.graph_hits > 0 and len(r.graphs) == len(r0.graphs) and len(r.proc_graphs) == len(r0.proc_graphs)
    assert r0.lp_steps == 0 and r0.lp is None  # a plain-only run never allocates the logprob buffers
    assert eng.kvm.num_free() == eng.num_blocks
    assert eng.runner.kernel_fault() == 0


@pytest.mark.parametrize("kw", [dict(enforce_eager=True), dict(async_scheduling=False)], ids=["eager", "sync"])
def test_engine_eager_and_synchronous_give_the_same_entries(graph_runs, kw):
    _, a, _, _ = graph_runs
    eng = _engine(**kw)
    c = _run(eng, True)
    for k in PROMPTS:
        assert c[k].output_ids == a[k].output_ids, k
    check_entries(c["q0"], 5)
    assert [(t, [i for i, _ in top]) for t, _, top in c["q0"].logprobs] == \
        [(t, [i for i, _ in top]) for t, _, top in a["q0"].logprobs]
    assert c["q1"].logprobs is None and [t for t, _, _ in c["q2"].logprobs] == [X] * 12
    assert eng.runner.lp_steps > 0 and (not kw.get("enforce_eager") or not eng.runner.graphs)
