"""Qwen3 (QK-norm) on the MI355X: the qk_norm_rope_kv kernel per element and the scope of its reduction,
then the tiny-qwen3 engine (graph == eager == reference, mixed / long steps, AWQ) and the real Qwen3
shapes. The CPU side (formula, config, oracle, fixture) is tests/test_qwen3_cpu.py."""
from __future__ import annotations

import pytest
import torch

import gemm_exact as X
import qwen3_cases as Q
from test_engine_gpu import _engine, _run
from test_gemm_exact_gpu import BF16, DEV, Guarded
from vgate import ops
from vgate.runtime.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

D, BS = Q.D, Q.BS


@pytest.fixture(autouse=True, scope="module")
def _native():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ops.native()
    yield


# ------------------------------------------------------------------ the kernel
def _launch(c, wide=40):
    """One launch on guarded operands: qkv inside guard rows (contiguous, as the op requires), q_out a
    strided view ``wide`` columns wider than Hq * 128, the caches between two guard blocks of sentinel."""
    T, Hq, Hkv = c["T"], c["Hq"], c["Hkv"]
    qg = Guarded(T, (Hq + 2 * Hkv) * D, init=c["qkv"], strided=False)
    og = Guarded(T, Hq * D + wide)
    kbig = torch.full((c["blocks"] + 2, Hkv, BS, D), X.SENT, dtype=BF16, device=DEV)
    vbig = kbig.clone()
    kc, vc = kbig[1:-1], vbig[1:-1]
    assert qg.view.is_contiguous() and kc.is_contiguous()
    ops.qk_norm_rope_kv(qg.view, c["positions"].to(DEV), c["slots"].to(DEV), c["cos_sin"].to(DEV), c["q_norm"].to(DEV),
                        c["k_norm"].to(DEV), Q.EPS, kc, vc, Hq, Hkv, og.view)
    torch.cuda.synchronize()
    what = f"T={T} Hq={Hq} Hkv={Hkv}"
    qg.assert_guards(what + " qkv")
    og.assert_guards(what + " q_out")
    assert torch.equal(qg.view.cpu(), c["qkv"]), what + ": qkv modified"                      # e
    assert bool((og.view[:, Hq * D:] == X.SENT).all()), what + ": q_out written past Hq * 128"
    for big in (kbig, vbig):                                                                  # d (guard blocks)
        assert bool((big[0] == X.SENT).all()) and bool((big[-1] == X.SENT).all()), what + ": cache guard"
    return og.view[:, : Hq * D].cpu().reshape(T, Hq, D), kc.cpu(), vc.cpu()


SHAPES = [(11, 3, 2),   # 5 heads: a partly idle wave
          (5, 16, 8),   # 24 heads: a second 16-head pass that is half idle
          (1, 1, 1)]


@pytest.mark.parametrize("exact_table", [True, False])
@pytest.mark.parametrize("T,Hq,Hkv", SHAPES)
def test_kernel_per_element(T, Hq, Hkv, exact_table):
    """a. {0, +1, -1} table: the rotation is a signed permutation of the normed values, every q and k element
    within 2^-8 |y64| (one bf16 rounding, 2^-9, doubled). b. real table: within 2^-8 (|a c| + |b s|), the same
    rounding bounded through the cancellation. c. V rows bit-equal. d. unwritten cache elements and every
    guard still the sentinel. e. qkv bit-unchanged (d, e and the guards: _launch)."""
    c = Q.make_case(T, Hq, Hkv, exact_table=exact_table)
    e = Q.expect64(c)
    q, kc, vc = _launch(c)
    w = Q.written(c)
    if exact_table:
        assert torch.equal(e["cancel_q"], e["q"].abs())  # no cancellation: one product is zero
        bq, bk = 2.0 ** -8 * e["q"].abs(), 2.0 ** -8 * e["k"].abs()
    else:
        bq, bk = 2.0 ** -8 * e["cancel_q"], 2.0 ** -8 * e["cancel_k"]
    Q.within(q, e["q"], bq, "q")
    Q.within(Q.cache_rows(kc, c), e["k"][w], bk[w], "k")
    assert torch.equal(vc.double(), e["v_cache"])                                             # c (+ d for V)
    unwritten = e["k_cache"] == X.SENT
    assert bool((kc.double()[unwritten] == X.SENT).all())                                     # d
    assert bool(unwritten.any()) and (len(w) < T or T == 1)  # some slots, and some tokens, really are unwritten


def _rms(t):
    return t.double().pow(2).mean(-1).sqrt()


def test_reduction_stays_inside_its_head():
    """Head h of token t holds values of magnitude 2^h * 8^(t % 3); gamma = 1 and the exact table make the
    output the normed input up to a signed permutation, so every head has unit RMS (within 2^-7: the
    per-element rounding is 2^-9). A sum of squares that took in a neighbouring head, DPP row or token would
    be off by a factor of 2 or more."""
    T, Hq, Hkv = 11, 3, 2
    c = Q.make_case(T, Hq, Hkv, exact_table=True)
    g = X._gen(4242)
    x = torch.randn(T, Hq + 2 * Hkv, D, generator=g)
    scale = 2.0 ** torch.arange(Hq + 2 * Hkv).clamp(max=Hq + Hkv - 1)[None, :, None] \
        * 8.0 ** (torch.arange(T) % 3)[:, None, None]
    c["qkv"] = (x * scale).to(BF16).reshape(T, -1)
    c["q_norm"] = c["k_norm"] = torch.ones(D, dtype=BF16)
    q, kc, _ = _launch(c)
    k = Q.cache_rows(kc, c)
    for name, r in (("q", _rms(q)), ("k", _rms(k))):
        assert bool(((r - 1.0).abs() <= 2.0 ** -7).all()), (name, r)
    # the input RMS of neighbouring heads really differs by about 2
    rin = _rms(c["qkv"].reshape(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv])
    assert bool((rin[:, 1:] / rin[:, :-1] > 1.5).all())


def test_norm_before_rotation_and_each_gamma_on_its_heads():
    """gamma[i] != gamma[i + 64] and q_norm != k_norm with a real table: the kernel meets the per-element
    bound of the definition, and the definition with the norm weight applied after the rotation, or with the
    two weights exchanged, lies far outside that bound (so the bound tells them apart)."""
    T, Hq, Hkv = 11, 3, 2
    c = Q.make_case(T, Hq, Hkv, seed=5)
    c["q_norm"] = torch.cat([torch.full((64,), 1.0), torch.full((64,), 2.0)]).to(BF16)
    c["k_norm"] = torch.cat([torch.full((64,), 3.0), torch.full((64,), 0.5)]).to(BF16)
    e = Q.expect64(c)
    q, kc, _ = _launch(c)
    w = Q.written(c)
    k = Q.cache_rows(kc, c)
    Q.within(q, e["q"], 2.0 ** -8 * e["cancel_q"], "q")
    Q.within(k, e["k"][w], 2.0 ** -8 * e["cancel_k"][w], "k")
    # gamma after the rotation: rotate the unit-gamma norm, then scale
    ones = dict(c, q_norm=torch.ones(D, dtype=BF16), k_norm=torch.ones(D, dtype=BF16))
    e1 = Q.expect64(ones)
    after_q, after_k = e1["q"] * c["q_norm"].double(), e1["k"] * c["k_norm"].double()
    swapped = Q.expect64(dict(c, q_norm=c["k_norm"], k_norm=c["q_norm"]))
    for wrong_q, wrong_k in ((after_q, after_k), (swapped["q"], swapped["k"])):
        assert bool(((q.double() - wrong_q).abs() > 2.0 ** -8 * e["cancel_q"]).any())
        assert bool(((k.double() - wrong_k[w]).abs() > 2.0 ** -8 * e["cancel_k"][w]).any())


def test_binding_rejects_bad_operands():
    c = Q.make_case(4, 2, 1)
    T, Hq, Hkv = 4, 2, 1
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    kc = torch.zeros(c["blocks"], Hkv, BS, D, dtype=BF16, device=DEV)
    vc = kc.clone()
    q_out = torch.zeros(T, Hq * D, dtype=BF16, device=DEV)
    C = ops.native()

    def call(**kw):
        a = dict(qkv=dev["qkv"], positions=dev["positions"], slots=dev["slots"], cos_sin=dev["cos_sin"],
                 q_norm=dev["q_norm"], k_norm=dev["k_norm"], eps=Q.EPS, k_cache=kc, v_cache=vc, Hq=Hq, Hkv=Hkv,
                 q_out=q_out)
        a.update(kw)
        C.qk_norm_rope_kv(**a)

    call()
    torch.cuda.synchronize()
    for bad in (dict(Hq=3), dict(positions=dev["positions"][:3]), dict(slots=dev["slots"][:3]),
                dict(q_norm=dev["q_norm"][:64]), dict(k_norm=dev["k_norm"].float()),
                dict(cos_sin=dev["cos_sin"][:, :64].contiguous()), dict(k_cache=kc[:, :, :, :64].contiguous()),
                dict(q_out=q_out[:3]), dict(q_out=q_out[:, :128]), dict(qkv=dev["qkv"][:, :-8]),
                dict(q_norm=c["q_norm"])):
        with pytest.raises(RuntimeError):
            call(**bad)


# ------------------------------------------------------------------ the engine
def _q3(**kw):
    return _engine(model="tiny-qwen3", **kw)


def _assert_margin(model, prompt, out, what):
    logits = model.reference_logits(prompt + out[:-1])[len(prompt) - 1:]
    for t, tok in enumerate(out):
        assert Q.margin_ok(logits[t], tok), (what, t)


def test_engine_graph_eager_reference_hits_and_embeddings():
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    g_eng = _q3()
    assert g_eng.arch.qk_norm and all(L.qkv.layout == "plain" for L in g_eng.model.layers)
    g = _run(g_eng, [(k, v, sp) for k, v in Q.PROMPTS.items()])
    e_eng = _q3(enforce_eager=True)
    e = _run(e_eng, [(k, v, sp) for k, v in Q.PROMPTS.items()])
    for k in Q.PROMPTS:
        assert len(g[k].output_ids) == 12 and g[k].output_ids == e[k].output_ids, k
    for k, v in list(Q.PROMPTS.items())[:3]:
        _assert_margin(e_eng.model, v, g[k].output_ids, k)
    hits0 = g_eng.runner.graph_hits
    again = _run(g_eng, [(k + "b", v, sp) for k, v in Q.PROMPTS.items()])
    assert g_eng.runner.graph_hits > hits0
    for k in Q.PROMPTS:
        assert again[k + "b"].output_ids == g[k].output_ids, k
    # the embeddings path (return_hidden)
    ids = Q.PROMPTS["q3"]
    vec, n = g_eng.embed(prompt_ids=ids)
    v = torch.tensor(vec)
    ref = g_eng.model.reference_logits(ids, return_hidden=True).float().mean(0).cpu()
    assert n == len(ids) and abs(v.norm().item() - 1) < 1e-3
    assert torch.nn.functional.cosine_similarity(v, ref / ref.norm(), dim=0).item() > 0.995
    assert int(ops.fault_word(g_eng.model.device)[0].item()) == 0


def test_engine_mixed_and_long_steps():
    """A 300-token prompt (chunks of >= 128 rows: the prefill GEMM path into the plain QKV buffer) beside
    short requests that already decode while its later chunks are prefilled."""
    long_prompt = [3 + (j * 29) % 500 for j in range(300)]
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    reqs = [("long", long_prompt, sp)] + [(k, v, sp) for k, v in list(Q.PROMPTS.items())[:3]]
    eng = _q3()
    g = _run(eng, reqs)
    e = _run(_q3(enforce_eager=True), reqs)
    for rid, prompt, _ in reqs:
        assert len(g[rid].output_ids) == 6 and g[rid].output_ids == e[rid].output_ids, rid
    _assert_margin(eng.model, long_prompt, g["long"].output_ids, "long")
    _assert_margin(eng.model, Q.PROMPTS["q1"], g["q1"].output_ids, "q1")


def test_engine_awq():
    eng = _q3(quantization="awq")
    assert all(L.qkv.kind == "awq" and L.qkv.layout == "plain" for L in eng.model.layers)
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    reqs = [(k, v, sp) for k, v in list(Q.PROMPTS.items())[:3]]
    g = _run(eng, reqs)
    e = _run(_q3(quantization="awq", enforce_eager=True), reqs)
    for k, ids in list(Q.PROMPTS.items())[:3]:
        assert len(g[k].output_ids) == 12 and g[k].output_ids == e[k].output_ids, k
        _assert_margin(eng.model, ids, g[k].output_ids, k)


@pytest.mark.parametrize("model", ["Qwen/Qwen3-1.7B", "Qwen/Qwen3-0.6B"])
def test_real_shapes_run(model):
    """q_size == hidden_size (1.7B) and q_size != hidden_size at hidden 1024 (0.6B), two layers each."""
    eng = _engine(model=model, max_model_len=1024, num_kv_blocks=1024, arch_overrides={"num_layers": 2})
    assert eng.arch.qk_norm and eng.arch.num_layers == 2
    sp = SamplingParams(temperature=0.7, top_p=0.9, max_tokens=16, ignore_eos=True)
    out = _run(eng, [(f"r{i}", list(range(10, 40 + i)), sp) for i in range(8)])
    assert all(len(s.output_ids) == 16 for s in out.values())
    assert all(0 <= t < 151936 for s in out.values() for t in s.output_ids)
    torch.cuda.synchronize()
    assert int(ops.fault_word(eng.model.device)[0].item()) == 0
