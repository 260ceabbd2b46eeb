"""Logits processors on the MI355X: csrc/kernels/logits_proc.hip against the dense oracle bit for
bit (whole tensor, eager and replayed from a graph), and the engine with penalised requests across
scheduling modes (asynchronous: the newest token is resolved on the device) and capture modes."""
import pytest
import torch

from logits_proc_cases import PENDING, build_case
from vgate import ops
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPTS = {f"q{i}": [3 + (i * 31 + j * 17) % 500 for j in range(7 + 9 * i)] for i in range(6)}  # test_engine_gpu.py
LONG = [3 + (j * 17) % 500 for j in range(40)]
GUARD = 1234.5  # columns past the vocabulary of the padded logits buffer: never written


def _specs(S, V, flip):
    """Rows of one launch: entries per row from {0, 1, 255, 256, 257, 2100} (2100 unique tokens need
    a vocabulary above 2100), the four pending cases, an entry past the vocabulary, a row with only
    a pending token (0 entries, pending "none") and a plain row."""
    big = 2100 if V > 4096 else 300
    if S == 1:
        return [(big, "hist", 0, True)] if flip else [(257, "none", 1, False)]
    if S == 3:
        return [(0, "none", 0, False), (256, "bias", 2, True), None] if flip else \
            [(255, "hist", 1, False), None, (big, "absent", 0, True)]
    sizes = [0, 1, 255, 256, 257, big, 0, 1, 255, 256, 257, big, 37, 5]
    specs = [(n, PENDING[(i + flip) % 4], (i + flip) % 5, i % 3 == flip) for i, n in enumerate(sizes)]
    specs.insert(4 + flip, None)
    return specs  # 15 rows: the 16th is bucket padding


def _device_logits(c, S, V):
    buf = torch.full((S, V + 8), GUARD, device=DEV)
    buf[:, :V] = c.logits.to(DEV)
    return buf


@pytest.mark.parametrize("V", [512, 128256, 151936])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_kernel_equals_dense_oracle_eager_and_graph(S, V):
    a = build_case(7 + S, V, _specs(S, V, 0), device=DEV, bucket=S)
    buf = _device_logits(a, S, V)
    lg = buf[:, :V]  # row stride above V, as the LM head's padded output
    prev = a.prev.to(DEV)
    pv = a.pm.view(S)
    assert ops.process_logits(lg, pv, prev) is lg
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), a.expected), [s for s in range(S) if not torch.equal(lg[s].cpu(), a.expected[s])]
    assert bool((buf[:, V:] == GUARD).all())
    assert not torch.equal(a.expected, a.logits)
    # captured launch, replayed on other buffer contents (same addresses)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.process_logits(lg, pv, prev)
    torch.cuda.current_stream().wait_stream(side)
    b = build_case(70 + S, V, _specs(S, V, 1), device=DEV, pm=a.pm, k=1, bucket=S)
    buf[:, :V] = b.logits.to(DEV)
    prev.copy_(b.prev)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), b.expected), [s for s in range(S) if not torch.equal(lg[s].cpu(), b.expected[s])]
    assert bool((buf[:, V:] == GUARD).all())


def test_kernel_without_prev_ignores_pending_words():
    """No previous sampler output (the first step, the CPU-style synchronous call): pend is not read."""
    c = build_case(3, 512, [(37, "absent", 0, False), None], device=DEV)
    c.pm._h[0]["pend"][:2] = -1
    c.pm.upload(0)
    lg = c.logits.to(DEV)
    ops.process_logits(lg, c.pm.view(2), None)
    assert torch.equal(lg.cpu(), c.expected)


# ------------------------------------------------------------------------------------- engine
def _engine(defer_capture=False, **kw):
    cfg = dict(model="tiny", device="cuda", max_model_len=512, max_num_seqs=16, max_num_batched_tokens=256,
               num_kv_blocks=256, warmup=False, seed=0)
    cfg.update(kw)
    eng = LLMEngine(EngineConfig(**cfg))
    eng.runner.defer_capture = defer_capture
    return eng


def _run(eng, reqs):
    done = {}

    def cb(kind, seq, payload):
        done[seq.request_id] = seq

    for rid, ids, sp in reqs:
        eng.add_request(rid, params=sp, callback=cb, prompt_ids=ids)
    eng.run_until_idle()
    return done


def _mixed_requests():
    """Penalised and plain requests, greedy and seeded sampled rows; the plain ones run longer, so
    the tail of the run is plain steps again."""
    g = dict(temperature=0.0, ignore_eos=True)
    s = dict(temperature=0.8, top_p=0.9, top_k=50, ignore_eos=True)
    sps = [SamplingParams(max_tokens=16, repetition_penalty=1.3, **g),
           SamplingParams(max_tokens=16, presence_penalty=0.7, frequency_penalty=0.4, **g),
           SamplingParams(max_tokens=16, frequency_penalty=1.5, logit_bias={11: 3.0, 57: 3.0, 106: -2.0}, seed=11, **s),
           SamplingParams(max_tokens=24, **g),
           SamplingParams(max_tokens=24, seed=5, **s),
           SamplingParams(max_tokens=16, repetition_penalty=1.2, presence_penalty=-0.3, seed=23, **s)]
    return [(k, v, sp) for (k, v), sp in zip(PROMPTS.items(), sps)]


@pytest.fixture(scope="module")
def mixed_async_graph():
    eng = _engine()
    assert eng.async_sched
    return eng, _run(eng, _mixed_requests())


def test_engine_async_equals_sync(mixed_async_graph):
    eng, a = mixed_async_graph
    sync = _engine(async_scheduling=False)
    b = _run(sync, _mixed_requests())
    for k in PROMPTS:
        assert a[k].output_ids == b[k].output_ids, k
    assert eng.runner.proc_steps > 0 and sync.runner.proc_steps == eng.runner.proc_steps
    assert eng.kvm.num_free() == eng.num_blocks and sync.kvm.num_free() == sync.num_blocks


def test_engine_graph_equals_eager_and_graph_tables(mixed_async_graph):
    eng, a = mixed_async_graph
    eager = _engine(enforce_eager=True)
    b = _run(eager, _mixed_requests())
    for k in PROMPTS:
        assert a[k].output_ids == b[k].output_ids, k
    r = eng.runner
    assert r.proc_graphs and all(g.vg_proc for g in r.proc_graphs.values())
    assert r.graphs and not any(g.vg_proc for g in r.graphs.values())  # the plain tail of the run
    assert not eager.runner.proc_graphs and not eager.runner.graphs
    snap = eng.snapshot()
    assert snap["proc_steps"] == r.proc_steps and snap["proc_graphs_captured"] == len(r.proc_graphs)


def test_deferred_capture_fills_the_processor_table():
    """Serving default: a first-seen processor bucket runs eagerly and is captured at idle on padding
    metadata with an all-empty processor header; its replays then serve real rows. The inputs take
    turns by output counts (six tokens at +30, frequency penalty 3), so the tokens do not hinge on
    near-ties of the tiny model's flat logits when the second request prefills from the prefix cache."""
    eng = _engine(defer_capture=True)
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True, frequency_penalty=3.0,
                        logit_bias={t: 30.0 for t in (11, 57, 106, 230, 371, 498)})
    first = _run(eng, [("a", LONG, sp)])["a"].output_ids  # eager steps, captured by run_until_idle
    r = eng.runner
    assert r.proc_graphs and not r.proc_pending and not r.graphs
    assert sorted(first.count(t) for t in sp.logit_bias) == [2] * 6
    hits = r.graph_hits
    again = _run(eng, [("c", LONG, sp)])["c"].output_ids
    assert again == first
    assert r.graph_hits > hits and not r.graphs


@pytest.mark.parametrize("freq", [30.0, 5.0])
def test_pending_token_is_counted_on_the_device(freq):
    """Two tokens biased by +100 under a frequency penalty above their base gap (the tiny model's
    logits span under 3): they must take turns, |count_A - count_B| <= 1 after every token. A count
    that is one step stale (the in-flight token not counted on the device) emits the same token twice
    in a row at once.

    How long the pair can hold the argmax is arithmetic: a biased token with c occurrences stands at
    about 100 - freq * c, an unbiased one at most at 1.2. freq = 5: 100 - 5 * 12 = 40, so all 24 tokens
    are A or B. freq = 30: 100 - 30 * 3 = 10 still wins, 100 - 30 * 4 = -20 never does, so exactly
    the first 8 tokens are A or B (4 each); from then on every emitted token drops by 30 and cannot
    come back, so tokens 9..24 are pairwise distinct and outside {A, B} (a stale count would repeat
    one immediately there as well)."""
    A, B = 123, 321
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, frequency_penalty=freq,
                        logit_bias={A: 100.0, B: 100.0})
    eng = _engine()
    assert eng.async_sched
    out = _run(eng, [("p", LONG, sp), ("q", PROMPTS["q2"], sp)])
    turns = 24 if freq == 5.0 else 8
    for k in ("p", "q"):
        toks = out[k].output_ids
        assert len(toks) == 24 and set(toks[:turns]) == {A, B}, toks
        for n in range(1, turns + 1):
            assert abs(toks[:n].count(A) - toks[:n].count(B)) <= 1, (k, n, toks)
        tail = toks[turns:]
        assert len(set(tail)) == len(tail) and not {A, B} & set(tail), toks
    assert eng.runner.proc_graphs and eng.kvm.num_free() == eng.num_blocks


def test_frequency_penalty_makes_outputs_distinct_and_frees_kv():
    eng = _engine()
    plain = _run(eng, [("p", LONG, SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True))])["p"].output_ids
    assert len(set(plain)) < 32
    sp = SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True, frequency_penalty=8.0)
    out = _run(eng, [("f", LONG, sp)])["f"].output_ids
    assert len(out) == 32 and len(set(out)) == 32
    assert eng.kvm.num_free() == eng.num_blocks
