"""Logprobs without a GPU: the float64 oracle itself, the CPU engine end to end (the CPU tier runs
``ops.logprobs`` on the logits its sampler reads), the chat API on both lanes, workers, SDK,
engine-process mode and the tensor-parallel refusal."""
import asyncio
import json
import threading

import httpx
import pytest
import torch

from logprobs_cases import check_entries
from vgate.api.app import ChatCompletionRequest, create_app
from vgate.backends.base import DryRunBackend
from vgate.backends.native import NativeBackend
from vgate.backends.remote import RemoteBackend
from vgate.cache import ResultCache
from vgate.config import VGateConfig, WorkerConfig
from vgate.engine import VGateEngine
from vgate.ops import reference as ref
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams

BODY = {"model": "m", "messages": [{"role": "user", "content": "hi"}]}
MSG = [{"role": "user", "content": "hi"}]
PROMPT = [5 + (j * 11) % 400 for j in range(16)]
CFG = dict(model="tiny", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
           num_kv_blocks=128, warmup=False, seed=0)
X = 77  # the biased token of the "after processors" cases


# ------------------------------------------------------------------------------------ the oracle
def test_reference_equals_torch_log_softmax():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 333, generator=g) * 7
    tok = torch.tensor([0, 332, 17, 400, -2], dtype=torch.int32)  # the last two are clamped
    k = torch.tensor([20, 5, 0, 1, -1], dtype=torch.int32)
    chosen, ids, lps = ref.logprobs_ref(x, tok, k)
    want = torch.log_softmax(x.double(), -1)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices
    for r in range(5):
        kk = int(k[r])
        if kk < 0:
            assert float(chosen[r]) == 0.0 and bool((ids[r] == -1).all()) and bool((lps[r] == 0).all())
            continue
        assert float(chosen[r]) == float(want[r, int(tok[r].clamp(0, 332))])
        assert ids[r, :kk].tolist() == order[r, :kk].tolist()
        assert torch.equal(lps[r, :kk], want[r, order[r, :kk]])
        assert bool((ids[r, kk:] == -1).all()) and bool((lps[r, kk:] == 0).all())
    assert abs(float(torch.logsumexp(want, -1).abs().max())) < 1e-12


def test_tie_rule_is_a_stable_sort_on_value_then_id():
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 8, (4, 257), generator=g).float() / 4
    x[0, 5], x[0, 3] = -0.0, 0.0  # equal values whatever the sign bit
    _, ids, lps = ref.logprobs_ref(x, torch.zeros(4, dtype=torch.int32), torch.full((4,), 20, dtype=torch.int32))
    for r in range(4):
        want = sorted(range(257), key=lambda i: (-float(x[r, i]), i))[:20]
        assert ids[r].tolist() == want
        assert all(a >= b for a, b in zip(lps[r].tolist(), lps[r].tolist()[1:]))


def test_minus_infinity_entries_rank_last():
    x = torch.tensor([[0.5, float("-inf"), 1.5, float("-inf"), -2.0]])
    chosen, ids, lps = ref.logprobs_ref(x, torch.tensor([3], dtype=torch.int32), torch.tensor([20], dtype=torch.int32))
    assert ids[0, :5].tolist() == [2, 0, 4, 1, 3] and bool((ids[0, 5:] == -1).all())
    assert float(chosen[0]) == float("-inf")
    assert lps[0, 3:5].tolist() == [float("-inf")] * 2 and bool(torch.isfinite(lps[0, :3]).all())
    assert abs(float(lps[0, :3].exp().sum()) - 1.0) < 1e-12


def test_sampling_params_validation():
    assert SamplingParams().logprobs is None
    for k in (0, 1, 20):
        assert SamplingParams(logprobs=k).logprobs == k
    for bad in (-1, 21, 2.5, True, "3"):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad)
    assert NativeBackend._params({"logprobs": 4}).logprobs == 4 and NativeBackend._params({}).logprobs is None


# ----------------------------------------------------------------------------------- CPU engine
def _run(eng, reqs):
    done = {}
    for rid, sp in reqs:
        eng.add_request(rid, params=sp, prompt_ids=PROMPT, callback=lambda k, s, p: done.update({s.request_id: s}))
    eng.run_until_idle()
    return done


def _greedy(**kw):
    return SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True, **kw)


@pytest.fixture(scope="module")
def cpu_run():
    eng = LLMEngine(EngineConfig(**CFG))
    done = _run(eng, [("lp", _greedy(logprobs=5)), ("plain", _greedy()),
                      ("bias", _greedy(logprobs=3, logit_bias={X: 100.0})), ("zero", _greedy(logprobs=0))])
    return eng, done


def test_engine_entries_are_consistent(cpu_run):
    eng, done = cpu_run
    check_entries(done["lp"], 5)
    assert done["lp"].output_ids == done["plain"].output_ids and len(done["plain"].output_ids) == 8
    assert done["plain"].logprobs is None
    assert eng.runner.lp_steps > 0 and eng.snapshot()["lp_steps"] == eng.runner.lp_steps


def test_engine_reports_the_distribution_after_the_processors(cpu_run):
    _, done = cpu_run
    assert done["bias"].output_ids == [X] * 8
    for tid, lp, top in done["bias"].logprobs:
        assert tid == X and lp > -1e-3 and top[0][0] == X and len(top) == 3


def test_engine_logprobs_zero_has_no_alternatives(cpu_run):
    _, done = cpu_run
    assert done["zero"].output_ids == done["plain"].output_ids
    assert [(t, top) for t, _, top in done["zero"].logprobs] == [(t, []) for t in done["plain"].output_ids]
    assert [lp for _, lp, _ in done["zero"].logprobs] == [lp for _, lp, _ in done["lp"].logprobs]


def test_engine_stop_string_and_eos_trim_entries(cpu_run):
    eng, done = cpu_run
    stop = eng.tokenizer.decode(done["plain"].output_ids[2:3])
    assert stop and stop not in eng.tokenizer.decode(done["plain"].output_ids[:2])
    eos = eng.arch.eos_token_ids[0]
    out = _run(eng, [("stop", SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True, stop=[stop], logprobs=2)),
                     ("eos", SamplingParams(temperature=0.0, max_tokens=8, logprobs=2, logit_bias={eos: 100.0}))])
    s = out["stop"]
    assert s.finish_reason == "stop" and s.output_ids == done["plain"].output_ids[:3]
    assert [t for t, _, _ in s.logprobs] == s.output_ids
    e = out["eos"]  # the EOS that ends the generation is stripped from the text: no entry
    assert e.finish_reason == "stop" and e.output_ids == [eos] and e.text == "" and e.logprobs == []
    res = NativeBackend._result(e)
    assert res["logprobs"] == [] and "logprobs" not in NativeBackend._result(done["plain"])


def test_runner_buffers_only_exist_after_a_logprob_step():
    eng = LLMEngine(EngineConfig(**CFG))
    _run(eng, [("plain", _greedy())])
    assert eng.runner.lp_steps == 0 and eng.runner.lp is None
    _run(eng, [("lp", _greedy(logprobs=1))])
    assert eng.runner.lp_steps == 8 and eng.runner.lp is not None


def test_engine_process_returns_the_same_entries(cpu_run):
    from vgate.runtime.engine_process import EngineProcessClient
    _, done = cpu_run
    cli = EngineProcessClient(EngineConfig(**CFG))
    try:
        res, ev = {}, threading.Event()

        def cb(kind, seq, payload):
            if kind != "token":
                res["seq"] = (kind, seq)
                ev.set()
        cli.add_request("lp", prompt_ids=PROMPT, params=_greedy(logprobs=5), callback=cb)
        assert ev.wait(120)
        kind, sv = res["seq"]
        assert kind == "finish" and sv.output_ids == done["lp"].output_ids
        alone = _run(LLMEngine(EngineConfig(**CFG)), [("lp", _greedy(logprobs=5))])["lp"]  # the same lone request
        assert [(t, lp, [tuple(a) for a in top]) for t, lp, top in sv.logprobs] == alone.logprobs
        out = NativeBackend._result(sv)["logprobs"]  # annotated with the core tokenizer's bytes
        assert [e["token_id"] for e in out] == sv.output_ids and \
            all(bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"] for e in out)
        bad = SamplingParams(logprobs=5)
        cli.cfg.tensor_parallel_size = 2  # the client applies the engine's admission check before the pipe
        try:
            with pytest.raises(ValueError, match="tensor parallel"):
                cli.add_request("bad", prompt_ids=PROMPT, params=bad)
        finally:
            cli.cfg.tensor_parallel_size = 1
    finally:
        cli.stop()


# ------------------------------------------------------------------------------------------ API
class Recording(DryRunBackend):
    def __init__(self):
        self.seen = []

    def create_sampling_params(self, temperature, top_p, max_tokens, **extra):
        self.seen.append(dict(extra))
        return {"temperature": temperature, "top_p": top_p, "max_tokens": max_tokens, **extra}

    async def agenerate(self, prompt, sp):
        return {"text": "out", "num_tokens": 2, "prompt_tokens": 1, "finish_reason": "length", "metrics": {}}


def make(backend, fast_lane=True, **cfg):
    c = VGateConfig(**cfg)
    eng = VGateEngine(model_config=c.model, worker_config=c.worker, backend=backend, dry_run=True)
    return create_app(c, engine=eng, fast_lane=fast_lane)


async def _http(app, fn):
    async with app.router.lifespan_context(app):
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as c:
            return await fn(c)


def test_request_model_and_cache_keys():
    assert ChatCompletionRequest(**BODY).extra() == {}
    assert ChatCompletionRequest(**BODY, logprobs=False).extra() == {}
    assert ChatCompletionRequest(**BODY, logprobs=True).extra() == {"logprobs": 0}
    assert ChatCompletionRequest(**BODY, logprobs=True, top_logprobs=7).extra() == {"logprobs": 7}
    import hashlib
    base = ResultCache.make_key("p", .7, .9, 64, extra=ChatCompletionRequest(**BODY).extra() or None)
    blob = json.dumps({"prompt": "p", "temperature": 0.7, "top_p": 0.9, "max_tokens": 64}, sort_keys=True)
    assert base == hashlib.sha256(blob.encode("utf-8")).hexdigest()[:16]  # a default request: today's key
    keys = {base} | {ResultCache.make_key("p", .7, .9, 64, extra=ChatCompletionRequest(
        **BODY, logprobs=True, top_logprobs=k).extra()) for k in (0, 1, 5, 20)}
    assert len(keys) == 5


@pytest.mark.parametrize("fast_lane", [True, False])
async def test_dry_run_answers_null_and_default_bodies_are_unchanged(fast_lane, monkeypatch):
    monkeypatch.setattr("vgate.api.app.os.urandom", lambda n: b"\x01" * n)
    monkeypatch.setattr("vgate.api.app.time.time", lambda: 1700000000)
    be = Recording()

    async def go(c):
        r = await c.post("/v1/chat/completions", json=BODY)
        today = json.dumps({
            "id": "chatcmpl-01010101", "object": "chat.completion", "created": 1700000000, "model": "m",
            "choices": [{"index": 0, "message": {"role": "assistant", "content": "out"}, "finish_reason": "length"}],
            "usage": {"prompt_tokens": 1, "completion_tokens": 2, "total_tokens": 3}}).encode()
        assert r.status_code == 200 and r.content == today
        r = await c.post("/v1/chat/completions", json=dict(BODY, logprobs=False))
        assert r.content == today
        r = await c.post("/v1/chat/completions", json=dict(BODY, logprobs=True, top_logprobs=3))
        ch = r.json()["choices"][0]
        assert r.status_code == 200 and "logprobs" in ch and ch["logprobs"] is None
        for bad in ({"top_logprobs": 2}, {"logprobs": False, "top_logprobs": 2}, {"logprobs": True, "top_logprobs": 21},
                    {"logprobs": True, "top_logprobs": -1}, {"logprobs": True, "stream": True}):
            r = await c.post("/v1/chat/completions", json=dict(BODY, **bad))
            assert r.status_code == 422, (bad, r.status_code, r.text)
        assert "out of scope" in r.text  # streaming logprobs: said in the error
    await _http(make(be, fast_lane=fast_lane, cache={"enabled": False}), go)
    assert be.seen == [{}, {}, {"logprobs": 3}]


@pytest.fixture(scope="module")
def native_backend():
    be = NativeBackend.__new__(NativeBackend)
    be.watchdog_seconds = 60.0
    be.engine = LLMEngine(EngineConfig(**CFG))
    be.engine.start()
    yield be
    be.engine.tp.size = 1
    be.engine.stop()


async def test_native_engine_through_both_lanes(native_backend, monkeypatch):
    monkeypatch.setattr("vgate.api.app.os.urandom", lambda n: b"\x01" * n)
    monkeypatch.setattr("vgate.api.app.time.time", lambda: 1700000000)
    body = dict(BODY, max_tokens=6, temperature=0.0, logprobs=True, top_logprobs=5)
    out = []
    for fast in (True, False):
        async def go(c):
            return [(r.status_code, r.content) for r in [
                await c.post("/v1/chat/completions", json=body),
                await c.post("/v1/chat/completions", json=dict(body, top_logprobs=0)),
                await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=6, temperature=0.0)),
                await c.post("/v1/chat/completions", json=dict(body, top_logprobs=30))]]
        out.append(await _http(make(native_backend, fast_lane=fast, cache={"enabled": False}), go))
    assert out[0] == out[1]  # the fast lane and the FastAPI route: identical bytes
    assert [s for s, _ in out[0]] == [200, 200, 200, 422]
    full, zero, plain = (json.loads(b) for _, b in out[0][:3])
    assert "logprobs" not in plain["choices"][0]
    content = full["choices"][0]["logprobs"]["content"]
    text = full["choices"][0]["message"]["content"]
    assert len(content) == full["usage"]["completion_tokens"] == 6 and text == plain["choices"][0]["message"]["content"]
    assert "".join(e["token"] for e in content) == text
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and len(e["top_logprobs"]) == 5
        assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
        first = e["top_logprobs"][0]  # temperature 0: the first alternative is the generated token
        assert (first["token"], first["logprob"], first["bytes"]) == (e["token"], e["logprob"], e["bytes"])
        for t in e["top_logprobs"]:
            assert set(t) == {"token", "logprob", "bytes"} and bytes(t["bytes"]).decode("utf-8", errors="replace") == t["token"]
    z = zero["choices"][0]["logprobs"]["content"]
    assert [(e["token"], e["logprob"]) for e in z] == [(e["token"], e["logprob"]) for e in content]
    assert all(e["top_logprobs"] == [] for e in z)


async def test_minus_infinity_is_written_as_minus_9999(native_backend):
    from vgate import logprobs as L
    assert L.result_entries([(3, float("-inf"), [(4, -0.5), (3, float("-inf"))])]) == \
        [{"token_id": 3, "logprob": -9999.0, "top": [[4, -0.5], [3, -9999.0]]}]
    tok = native_backend.engine.tokenizer
    e = L.annotate(L.result_entries([(300, -1.0, [(301, -2.0)])]), lambda t: tok.decode_bytes([t]))
    c = L.content(e)[0]
    assert c["token"] == tok.decode([300]) and c["top_logprobs"][0]["token"] == tok.decode([301])
    json.dumps(c, allow_nan=False)


async def test_tensor_parallel_is_refused_with_400(native_backend):
    async def go(c):
        native_backend.engine.tp.size = 2
        try:
            r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=2, logprobs=True))
        finally:
            native_backend.engine.tp.size = 1
        assert r.status_code == 400 and "tensor parallel" in r.json()["detail"], r.text
        r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=2, logprobs=True))
        assert r.status_code == 200 and len(r.json()["choices"][0]["logprobs"]["content"]) == 2
    await _http(make(native_backend, cache={"enabled": False}), go)


# ------------------------------------------------------------------------------- workers and SDK
async def test_worker_route_carries_the_field_and_annotates_results(native_backend):
    seen = []

    def handler(request):
        body = json.loads(request.content)
        seen.append(body)
        return httpx.Response(200, json={"results": [{"text": p, "num_tokens": 1} for p in body["prompts"]]})
    be = RemoteBackend(WorkerConfig(endpoints=["http://a:8001"]), transport=httpx.MockTransport(handler))
    await be.agenerate("p", be.create_sampling_params(temperature=0.0, top_p=0.8, max_tokens=4))
    await be.agenerate("p", be.create_sampling_params(temperature=0.0, top_p=0.8, max_tokens=4, logprobs=2))
    await be.aclose()
    assert seen[0]["sampling_params"] == {"temperature": 0.0, "top_p": 0.8, "max_tokens": 4}  # no new key
    assert seen[1]["sampling_params"] == {"temperature": 0.0, "top_p": 0.8, "max_tokens": 4, "logprobs": 2}

    async def go(c):
        res = []
        for body in seen:
            r = await c.post("/internal/generate", json=body)
            assert r.status_code == 200, r.text
            res.append(r.json()["results"][0])
        return res
    plain, lp = await _http(make(native_backend, role="worker"), go)
    assert "logprobs" not in plain and len(lp["logprobs"]) == 4
    for e in lp["logprobs"]:  # the worker owns the tokenizer: the gateway needs none
        assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"] and len(e["top"]) == len(e["top_tokens"]) == 2
    from vgate.logprobs import content
    assert [c["token"] for c in content(lp["logprobs"])] == [e["token"] for e in lp["logprobs"]]


def test_sdk_bodies_and_models():
    from vgate_client import AsyncVGate, VGate
    from vgate_client.exceptions import VGateError
    bodies = []
    entry = {"token": " ka", "logprob": -0.25, "bytes": [32, 107, 97],
             "top_logprobs": [{"token": " ka", "logprob": -0.25, "bytes": [32, 107, 97]},
                              {"token": "x", "logprob": -9999.0, "bytes": [120]}]}

    def handler(request):
        bodies.append(json.loads(request.content))
        b = bodies[-1]
        if b.get("logprobs") and b["stream"]:
            return httpx.Response(422, json={"detail": "logprobs with stream: true is not supported"})
        if b["stream"]:
            return httpx.Response(200, content=b"data: [DONE]\n\n", headers={"content-type": "text/event-stream"})
        choice = {"index": 0, "message": {"role": "assistant", "content": " ka"}, "finish_reason": "stop"}
        if b.get("logprobs"):
            choice["logprobs"] = {"content": [entry]} if b.get("top_logprobs") else None
        return httpx.Response(200, json={"id": "c", "object": "chat.completion", "created": 1, "model": "m",
                                         "choices": [choice],
                                         "usage": {"prompt_tokens": 1, "completion_tokens": 1, "total_tokens": 2}})
    c = VGate(base_url="http://t", transport=httpx.MockTransport(handler), max_retries=0)
    plain = c.chat.create(model="m", messages=MSG)
    full = c.chat.create(model="m", messages=MSG, logprobs=True, top_logprobs=2)
    null = c.chat.create(model="m", messages=MSG, logprobs=True)
    with pytest.raises(VGateError):
        list(c.chat.stream(model="m", messages=MSG, logprobs=True))
    c.close()

    async def go():
        a = AsyncVGate(base_url="http://t", transport=httpx.MockTransport(handler), max_retries=0)
        r = await a.chat.create(model="m", messages=MSG, logprobs=True, top_logprobs=2)
        with pytest.raises(VGateError):
            async for _ in a.chat.stream(model="m", messages=MSG, logprobs=True, top_logprobs=1):
                pass
        await a.close()
        return r
    afull = asyncio.run(go())
    base = {"model": "m", "messages": MSG, "temperature": 0.7, "top_p": 0.9, "max_tokens": 256, "stream": False}
    assert bodies[0] == base  # no new keys
    assert bodies[1] == dict(base, logprobs=True, top_logprobs=2) == bodies[4]
    assert bodies[2] == dict(base, logprobs=True) and bodies[3] == dict(base, stream=True, logprobs=True)
    assert bodies[5] == dict(base, stream=True, logprobs=True, top_logprobs=1)
    assert plain.choices[0].logprobs is None and null.choices[0].logprobs is None
    for r in (full, afull):
        lp = r.choices[0].logprobs.content
        assert len(lp) == 1 and lp[0].token == " ka" and lp[0].logprob == -0.25 and bytes(lp[0].bytes) == b" ka"
        assert [(t.token, t.logprob) for t in lp[0].top_logprobs] == [(" ka", -0.25), ("x", -9999.0)]
