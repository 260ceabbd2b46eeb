"""Logits processors (penalties, logit_bias) without a GPU: the sparse path (host state -> step
buffer -> ops.ref.process_logits_sparse, the algorithm of csrc/kernels/logits_proc.hip) against the
dense oracle bit for bit, and the engine on the CPU against a hand loop over the dense model."""
import pytest
import torch

from logits_proc_cases import PARAMS, PENDING, build_case
from vgate import ops
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.logits_proc import SeqProcState
from vgate.runtime.sampling_params import SamplingParams

PROMPTS = {f"q{i}": [3 + (i * 31 + j * 17) % 500 for j in range(7 + 9 * i)] for i in range(6)}  # test_engine_gpu.py
LONG = [3 + (j * 17) % 500 for j in range(40)]


def make_engine(**kw):
    cfg = dict(model="tiny", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
               num_kv_blocks=128, warmup=False, seed=0)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def collect(engine, reqs):
    done = {}

    def cb(kind, seq, payload):
        if kind in ("finish", "error"):
            done[seq.request_id] = seq

    for rid, ids, sp in reqs:
        engine.add_request(rid, params=sp, callback=cb, prompt_ids=ids)
    engine.run_until_idle()
    return done


# ------------------------------------------------------------------ sampling params / host state
def test_sampling_params_fields_and_validation():
    sp = SamplingParams()
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == (1.0, 0.0, 0.0, {})
    assert not sp.has_processors
    for kw in ({"repetition_penalty": 1.1}, {"presence_penalty": -0.5}, {"frequency_penalty": 0.1},
               {"logit_bias": {3: 0.0}}):
        assert SamplingParams(**kw).has_processors, kw
    assert SamplingParams(logit_bias={"5": 1}).logit_bias == {5: 1.0}
    for kw in ({"repetition_penalty": 0.0}, {"repetition_penalty": float("inf")}, {"presence_penalty": float("nan")},
               {"frequency_penalty": float("inf")}, {"logit_bias": {-1: 1.0}}):
        with pytest.raises(ValueError):
            SamplingParams(**kw)


def test_native_backend_params_reads_the_new_keys():
    from vgate.backends.native import NativeBackend
    sp = NativeBackend._params({"temperature": 0.0, "repetition_penalty": 1.2, "presence_penalty": 0.3,
                                "frequency_penalty": -0.1, "logit_bias": {"7": 2.5}, "seed": 4, "top_k": 9})
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty) == (1.2, 0.3, -0.1)
    assert sp.logit_bias == {7: 2.5} and sp.seed == 4 and sp.top_k == 9
    assert not NativeBackend._params({"temperature": 0.5}).has_processors


def test_state_counts_prompt_bit_and_growth():
    st = SeqProcState([5, 5, 9], {9: 1.5, 11: -2.0})
    e = {int(r["tok"]): (int(r["cnt"]) & 0x7FFFFFFF, int(r["cnt"]) < 0, float(r["bias"])) for r in st.entries()}
    assert e == {5: (0, True, 0.0), 9: (0, True, 1.5), 11: (0, False, -2.0)}
    for t in [5, 11, 11] + list(range(100, 300)):  # grows past its first allocation
        st.add_output(t)
    e = {int(r["tok"]): (int(r["cnt"]) & 0x7FFFFFFF, int(r["cnt"]) < 0) for r in st.entries()}
    assert e[5] == (1, True) and e[11] == (2, False) and e[9] == (0, True) and e[299] == (1, False)
    assert st.n == 203 and len({int(t) for t in st.entries()["tok"]}) == 203
    assert st.entries().dtype.itemsize == 16


# ------------------------------------------------------------------ sparse path == dense oracle
def _specs(V, sizes):
    specs = []
    for i, n in enumerate(sizes):
        specs.append((n, PENDING[i % 4], i % len(PARAMS), i % 3 == 1))
    specs.insert(2, None)  # a plain row in the middle
    return specs


@pytest.fixture
def one_torch_thread():
    """The big-vocabulary rows are the only tensors of this file large enough for torch's intra-op
    thread pool. Observed: when they use it late in a long pytest process (the whole CPU tier), every
    CPU-engine test after them runs ~100x slower; single-threaded they do not. The comparison needs no
    parallelism, so it stays on the calling thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("V", [512, 151936])
def test_sparse_path_equals_dense_oracle(V, one_torch_thread):
    sizes = [0, 1, 4, 37, 255, 256, 257, 300] + ([2100] if V > 4096 else [400])
    for seed in range(3):
        # every pending case meets every size / parameter set over the seeds
        specs = [None if sp is None else (sp[0], PENDING[(PENDING.index(sp[1]) + seed) % 4], (sp[2] + seed) % len(PARAMS), sp[3])
                 for sp in _specs(V, sizes)]
        c = build_case(100 + seed, V, specs, bucket=len(specs) + 2)
        before = c.logits.clone()
        got = ops.process_logits(c.logits, c.pm.view(c.logits.shape[0]), c.prev)
        assert torch.equal(c.logits, before)  # the CPU front end works on a copy
        assert torch.equal(got, c.expected), [s for s in range(len(specs)) if not torch.equal(got[s], c.expected[s])]
        plain = [s for s, sp in enumerate(specs) if sp is None] + list(range(len(specs), got.shape[0]))
        assert all(torch.equal(got[s], before[s]) for s in plain)  # empty rows: bit-identical
        assert not torch.equal(got, before)


def test_oracle_semantics_by_hand():
    """The dense oracle itself, on values worked out by hand (order of the four steps)."""
    x = torch.tensor([2.0, -2.0, 1.0, 1.0, 3.0])
    sp = SamplingParams(repetition_penalty=2.0, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={3: 1.0, 0: -1.0})
    out = ops.ref.process_logits_ref(x, prompt_ids=[0], output_ids=[1, 1, 2], params=sp)
    # tok0: prompt only: 2/2 - 1 = 0 ; tok1: c=2: -2*2 - .5 - .5 = -5 ; tok2: c=1: .5 - .25 - .5 = -.25
    # tok3: bias only: 2 ; tok4: untouched
    assert out.tolist() == [0.0, -5.0, -0.25, 2.0, 3.0]


# ------------------------------------------------------------------ engine on the CPU
def hand_loop(model, prompt, n, sp):
    ids, out = list(prompt), []
    for _ in range(n):
        row = model.reference_logits(ids)[-1]
        tok = int(torch.argmax(ops.ref.process_logits_ref(row, prompt, out, sp)))
        out.append(tok)
        ids.append(tok)
    return out


PARAM_SETS = {
    "repetition": dict(repetition_penalty=1.3),
    "presence_frequency": dict(presence_penalty=0.7, frequency_penalty=0.4),
    "bias": dict(logit_bias={11: 1.5, 106: -2.0, 30: -1.0, 400: 0.75}),
}


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_engine_tokens_equal_hand_loop(name):
    """Engine tokens == hand loop over the dense fp32 model, exactly, 24 greedy tokens per prompt.

    The engine runs with ``dtype="float32"``: the CPU reference path then keeps activations and the
    KV cache in fp32, as the oracle does, so the comparison checks the engine's logic (host state,
    packing, the sparse processor, scheduling) and nothing else. With the default bf16 activations
    (which mirror the GPU kernels' rounding) the tiny model's flat logits make exact equality a matter
    of rounding, with or without processors: measured on this tree, "repetition" and
    "presence_frequency" differ from the fp32 loop on q0, q4, q5 at steps where the oracle's two best
    processed logits are 0.00012 .. 0.00625 apart, and plain greedy requests differ in the same way
    on q2, q4, q5 (gaps 0.00012 .. 0.00073). The bf16 engine is checked step by step within the bf16
    margin by test_engine_tokens_track_hand_loop_teacher_forced."""
    eng = make_engine(dtype="float32")
    assert eng.kv_caches[0][0].dtype == torch.float32
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, **PARAM_SETS[name])
    out = collect(eng, [(k, v, sp) for k, v in PROMPTS.items()])
    for k, v in PROMPTS.items():
        assert out[k].output_ids == hand_loop(eng.model, v, 24, sp), (name, k)
    assert eng.runner.proc_steps > 0 and eng.snapshot()["proc_steps"] == eng.runner.proc_steps
    assert eng.kvm.num_free() == eng.num_blocks


def test_float32_cpu_engine_is_exact_and_default_stays_bf16():
    """EngineConfig.dtype: "float32" on the CPU reproduces the dense fp32 forward token for token over
    24 plain greedy tokens of every prompt; the default keeps bf16 activations and a bf16 KV cache."""
    eng = make_engine(dtype="float32")
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    out = collect(eng, [(k, v, sp) for k, v in PROMPTS.items()])
    for k, v in PROMPTS.items():
        ids, ref_toks = list(v), []
        for _ in range(24):
            ref_toks.append(int(torch.argmax(eng.model.reference_logits(ids)[-1])))
            ids.append(ref_toks[-1])
        assert out[k].output_ids == ref_toks, k
    assert eng.runner.proc_steps == 0
    default = make_engine()
    assert default.kv_caches[0][0].dtype == torch.bfloat16 and default.model.act_dtype == torch.bfloat16


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_engine_tokens_track_hand_loop_teacher_forced(name):
    """Teacher-forced on the engine's own tokens: every greedy choice is the argmax of the dense
    oracle's processed row up to the bf16 margin. Margin: the engine rounds the last layer's
    residual, norm output, attention output and MLP output to bf16 (unit round-off 2^-8) before the
    fp32 LM head, i.e. up to 4 * 2^-8 of the largest logit, which a repetition penalty scales by at
    most rep = 1.3. The penalties themselves (0.4 .. 1.5) are 20x larger: a missed, doubled or stale
    count moves the argmax far outside it."""
    eng = make_engine()
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, **PARAM_SETS[name])
    out = collect(eng, [(k, v, sp) for k, v in PROMPTS.items()])
    for k, v in PROMPTS.items():
        toks = out[k].output_ids
        assert len(toks) == 24
        rows = eng.model.reference_logits(v + toks[:-1])[len(v) - 1:]
        for t, tok in enumerate(toks):
            pr = ops.ref.process_logits_ref(rows[t], v, toks[:t], sp)
            tol = 1.3 * 4 * 2.0 ** -8 * float(rows[t].abs().max())
            assert float(pr[tok]) >= float(pr.max()) - tol, (name, k, t, float(pr.max()) - float(pr[tok]), tol)
    assert eng.runner.proc_steps > 0 and eng.snapshot()["proc_steps"] == eng.runner.proc_steps


# Decisive inputs for the run-to-run comparisons below: six tokens biased by +30 under a frequency
# penalty of 3 take turns by their output COUNTS (a gap of 3 per occurrence; 24 tokens = 4 turns each,
# 30 - 12 still far above every unbiased logit), so the tokens do not hinge on near-ties of the tiny
# model's flat logits (which a bf16 forward resolves differently when the same prompt is prefilled in
# another chunking: plain greedy requests show that too), and any lost or doubled count changes them.
TURNS = dict(frequency_penalty=3.0, repetition_penalty=1.3, logit_bias={t: 30.0 for t in (11, 57, 106, 230, 371, 498)})


def test_prefix_cache_hit_and_preemption_keep_tokens():
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, **TURNS)
    eng = make_engine()
    first = collect(eng, [("a", LONG, sp)])["a"].output_ids
    again = collect(eng, [("b", LONG, sp)])["b"]  # same prompt: served from the prefix cache
    assert again.num_cached_prefix > 0 and again.output_ids == first
    assert first == hand_loop(eng.model, LONG, 24, sp)
    assert sorted(first.count(t) for t in TURNS["logit_bias"]) == [4] * 6
    free = collect(make_engine(), [(k, v, sp) for k, v in PROMPTS.items()])
    tight = make_engine(num_kv_blocks=14)  # too few blocks for all six: recompute preemption
    got = collect(tight, [(k, v, sp) for k, v in PROMPTS.items()])
    assert tight.scheduler.num_preemptions > 0
    for k in PROMPTS:
        assert got[k].output_ids == free[k].output_ids, k
    assert tight.kvm.num_free() == tight.num_blocks


def test_frequency_penalty_makes_outputs_distinct():
    """The tiny model's fp32 logits span [-1.34, 1.18] on this prompt: a frequency penalty of 8 puts
    every generated token out of reach, so 32 greedy outputs are pairwise distinct; without it the
    greedy run repeats tokens."""
    plain = collect(make_engine(), [("p", LONG, SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True))])["p"]
    assert len(set(plain.output_ids)) < 32
    sp = SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True, frequency_penalty=8.0)
    out = collect(make_engine(), [("f", LONG, sp)])["f"].output_ids
    assert len(out) == 32 and len(set(out)) == 32


def test_logit_bias_forces_and_bans_tokens():
    A = 123
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True, logit_bias={A: 100.0})
    assert collect(make_engine(), [("a", LONG, sp)])["a"].output_ids == [A] * 12
    g = collect(make_engine(), [("g", LONG, SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True))])["g"].output_ids[0]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True, logit_bias={g: -100.0})
    assert g not in collect(make_engine(), [("b", LONG, sp)])["b"].output_ids


def test_plain_requests_run_no_processor_step_and_limits():
    eng = make_engine()
    collect(eng, [(k, v, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)) for k, v in PROMPTS.items()])
    assert eng.runner.proc_steps == 0 and eng.runner.procmeta is None
    with pytest.raises(ValueError):
        eng.add_request("x", prompt_ids=[1, 2], params=SamplingParams(logit_bias={eng.arch.vocab_size: 1.0}))
    eng.tp.size = 2  # a tensor-parallel group: processors are refused, plain requests are not
    try:
        with pytest.raises(ValueError):
            eng.add_request("y", prompt_ids=[1, 2], params=SamplingParams(presence_penalty=0.5))
    finally:
        eng.tp.size = 1
