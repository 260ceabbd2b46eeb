"""Sampling controls through the public interface (penalties, logit_bias, seed, top_k): requests
without them are served exactly as before (cache keys, worker bodies, SDK bodies, three-argument
backends); requests with them reach the backend, split the cache and the in-flight coalescing, and
are validated."""
import asyncio
import json

import httpx
import pytest

from vgate.api.app import create_app
from vgate.backends.base import DryRunBackend
from vgate.backends.remote import RemoteBackend
from vgate.batcher import RequestBatcher
from vgate.cache import ResultCache
from vgate.config import VGateConfig, WorkerConfig, set_config
from vgate.engine import VGateEngine

BODY = {"model": "m", "messages": [{"role": "user", "content": "hi"}]}
MSG = [{"role": "user", "content": "hi"}]
CONTROLS = {"presence_penalty": 0.5, "frequency_penalty": -0.25, "repetition_penalty": 1.2,
            "logit_bias": {"7": 2.5, "11": -100}, "seed": 3, "top_k": 40}
A = "http://a:8001"


class Recording(DryRunBackend):
    """Accepts the optional controls and records what create_sampling_params was given."""

    def __init__(self, delay=0.0):
        self.seen = []
        self.calls = 0
        self.delay = delay

    def create_sampling_params(self, temperature, top_p, max_tokens, **extra):
        self.seen.append(dict(extra))
        return {"temperature": temperature, "top_p": top_p, "max_tokens": max_tokens, **extra}

    async def agenerate(self, prompt, sp):
        self.calls += 1
        await asyncio.sleep(self.delay)
        return {"text": "out", "num_tokens": 2, "prompt_tokens": 1, "finish_reason": "length", "metrics": {}}

    async def stream_generate(self, prompt, sp):
        yield {"delta": "x", "num_tokens": 1, "finish_reason": "length"}


class ThreeArgs(Recording):
    def create_sampling_params(self, temperature, top_p, max_tokens):  # the form before this feature
        self.seen.append({})
        return {"temperature": temperature, "top_p": top_p, "max_tokens": max_tokens}


def make(backend, fast_lane=True, **cfg):
    c = VGateConfig(**cfg)
    eng = VGateEngine(model_config=c.model, worker_config=c.worker, backend=backend, dry_run=True)
    return create_app(c, engine=eng, fast_lane=fast_lane)


async def _run(app, fn):
    async with app.router.lifespan_context(app):
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as c:
            return await fn(c)


# ----------------------------------------------------------------------- defaults are unchanged
def test_cache_keys_of_default_requests_are_unchanged():
    import hashlib
    k = ResultCache.make_key("p", .7, .9, 64)
    assert k == ResultCache.make_key("p", .7, .9, 64, extra=None) == ResultCache.make_key("p", .7, .9, 64, extra={})
    blob = json.dumps({"prompt": "p", "temperature": 0.7, "top_p": 0.9, "max_tokens": 64}, sort_keys=True)
    assert k == hashlib.sha256(blob.encode("utf-8")).hexdigest()[:16]


def test_cache_key_differs_per_control_value():
    base = ResultCache.make_key("p", .7, .9, 64)
    keys = {base}
    for extra in ({"seed": 1}, {"seed": 2}, {"presence_penalty": 0.5}, {"presence_penalty": 0.6},
                  {"frequency_penalty": 0.5}, {"repetition_penalty": 1.1}, {"top_k": 5},
                  {"logit_bias": {"7": 1.0}}, {"logit_bias": {"7": 2.0}}, {"logit_bias": {"8": 1.0}},
                  {"seed": 1, "top_k": 5}):
        keys.add(ResultCache.make_key("p", .7, .9, 64, extra=extra))
    assert len(keys) == 12
    assert ResultCache.make_key("p", .7, .9, 64, extra={"seed": 1, "top_k": 5}) == \
        ResultCache.make_key("p", .7, .9, 64, extra={"top_k": 5, "seed": 1})


async def test_three_argument_backend_and_default_request_path():
    be = ThreeArgs()

    async def go(c):
        r = await c.post("/v1/chat/completions", json=BODY)
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] == "out"
        r = await c.post("/v1/chat/completions", json=dict(BODY, stream=True))
        assert r.status_code == 200 and "[DONE]" in r.text
    await _run(make(be, cache={"enabled": False}), go)
    assert be.seen == [{}, {}]


async def test_worker_body_and_worker_route():
    seen = []

    def handler(request):
        body = json.loads(request.content)
        seen.append(body)
        return httpx.Response(200, json={"results": [{"text": p, "num_tokens": 1} for p in body["prompts"]]})
    be = RemoteBackend(WorkerConfig(endpoints=[A]), transport=httpx.MockTransport(handler))
    await be.agenerate("p", be.create_sampling_params(temperature=0.3, top_p=0.8, max_tokens=17))
    extra = {"presence_penalty": 0.5, "logit_bias": {"7": 2.5}, "seed": 3}
    await be.agenerate("p", be.create_sampling_params(temperature=0.3, top_p=0.8, max_tokens=17, **extra))
    await be.aclose()
    assert seen[0]["sampling_params"] == {"temperature": 0.3, "top_p": 0.8, "max_tokens": 17}  # no new keys
    assert seen[1]["sampling_params"] == {"temperature": 0.3, "top_p": 0.8, "max_tokens": 17, **extra}
    # ... and the worker's route hands them to its backend
    wb = Recording()

    async def go(c):
        for sp in seen:
            r = await c.post("/internal/generate", json=sp)
            assert r.status_code == 200, r.text
    await _run(make(wb, role="worker"), go)
    assert wb.seen == [{}, {"presence_penalty": 0.5, "logit_bias": {7: 2.5}, "seed": 3}]


def test_sdk_bodies():
    from vgate_client import AsyncVGate, VGate
    bodies = []

    def handler(request):
        bodies.append(json.loads(request.content))
        if bodies[-1]["stream"]:
            return httpx.Response(200, content=b"data: [DONE]\n\n", headers={"content-type": "text/event-stream"})
        return httpx.Response(200, json={"id": "c", "object": "chat.completion", "created": 1, "model": "m",
                                         "choices": [{"index": 0, "message": {"role": "assistant", "content": "x"},
                                                      "finish_reason": "stop"}],
                                         "usage": {"prompt_tokens": 1, "completion_tokens": 1, "total_tokens": 2}})
    kw = dict(presence_penalty=0.5, frequency_penalty=-0.25, repetition_penalty=1.2, logit_bias={7: 2.5, "11": -100},
              seed=3, top_k=40)
    want = dict(kw, logit_bias={"7": 2.5, "11": -100.0})
    c = VGate(base_url="http://t", transport=httpx.MockTransport(handler))
    c.chat.create(model="m", messages=MSG)
    c.chat.create(model="m", messages=MSG, **kw)
    list(c.chat.stream(model="m", messages=MSG))
    list(c.chat.stream(model="m", messages=MSG, seed=9))
    c.close()

    async def go():
        a = AsyncVGate(base_url="http://t", transport=httpx.MockTransport(handler))
        await a.chat.create(model="m", messages=MSG)
        await a.chat.create(model="m", messages=MSG, **kw)
        async for _ in a.chat.stream(model="m", messages=MSG, top_k=2):
            pass
        await a.close()
    asyncio.run(go())
    plain = {"model": "m", "messages": MSG, "temperature": 0.7, "top_p": 0.9, "max_tokens": 256, "stream": False}
    assert bodies[0] == plain and bodies[4] == plain  # no new keys
    assert bodies[1] == dict(plain, **want) and bodies[5] == dict(plain, **want)
    assert bodies[2] == dict(plain, stream=True)
    assert bodies[3] == dict(plain, stream=True, seed=9) and bodies[6] == dict(plain, stream=True, top_k=2)


# ------------------------------------------------------------------------- the fields are honoured
@pytest.mark.parametrize("fast_lane", [True, False])
async def test_fields_reach_the_backend(fast_lane):
    be = Recording()

    async def go(c):
        r = await c.post("/v1/chat/completions", json=dict(BODY, **CONTROLS))
        assert r.status_code == 200, r.text
        r = await c.post("/v1/chat/completions", json=dict(BODY, stream=True, seed=5, top_k=2))
        assert r.status_code == 200 and "[DONE]" in r.text
        r = await c.post("/v1/chat/completions", json=BODY)
        assert r.status_code == 200
    await _run(make(be, fast_lane=fast_lane, cache={"enabled": False}), go)
    assert be.seen == [CONTROLS, {"seed": 5, "top_k": 2}, {}]


async def test_fast_lane_and_fastapi_route_give_the_same_bytes(monkeypatch):
    monkeypatch.setattr("vgate.api.app.os.urandom", lambda n: b"\x01" * n)
    monkeypatch.setattr("vgate.api.app.time.time", lambda: 1700000000)
    out = []
    for fast in (True, False):
        async def go(c):
            res = []
            for body in (dict(BODY, **CONTROLS), dict(BODY, presence_penalty=3.0), dict(BODY, logit_bias={"x": 1.0})):
                r = await c.post("/v1/chat/completions", json=body)
                res.append((r.status_code, r.content))
            return res
        out.append(await _run(make(Recording(), fast_lane=fast, cache={"enabled": False}), go))
    assert out[0] == out[1]
    assert [s for s, _ in out[0]] == [200, 422, 422]


async def test_requests_differing_in_seed_are_not_coalesced():
    set_config(VGateConfig(cache={"enabled": True, "maxsize": 100}))

    class _Engine:
        is_remote = False

    be = Recording(delay=0.02)
    eng = _Engine()
    eng.backend = be
    b = RequestBatcher(eng)
    await b.start()
    await asyncio.gather(b.submit("p", max_tokens=8, extra={"seed": 1}), b.submit("p", max_tokens=8, extra={"seed": 1}))
    assert be.calls == 1  # same controls: one inference
    await asyncio.gather(b.submit("p", max_tokens=8, extra={"seed": 2}), b.submit("p", max_tokens=8, extra={"seed": 3}),
                         b.submit("p", max_tokens=8))
    assert be.calls == 4
    await b.submit("p", max_tokens=8, extra={"seed": 2})  # served from the cache under its own key
    assert be.calls == 4
    assert be.seen == [{"seed": 1}, {"seed": 2}, {"seed": 3}, {}]
    await b.stop()


# --------------------------------------------------------------------------------- validation
BAD = [{"presence_penalty": 2.5}, {"presence_penalty": -2.1}, {"frequency_penalty": 2.01}, {"frequency_penalty": -3},
       {"repetition_penalty": 0}, {"repetition_penalty": -1.0}, {"repetition_penalty": 10.5},
       {"logit_bias": {"7": 101}}, {"logit_bias": {"7": -100.5}}, {"logit_bias": {"-3": 1.0}}, {"logit_bias": {"a": 1.0}},
       {"logit_bias": {"1.5": 1.0}}, {"logit_bias": {str(i): 0.5 for i in range(301)}}, {"logit_bias": [1, 2]},
       {"seed": -1}, {"top_k": 0}]
GOOD = [{"presence_penalty": 2.0, "frequency_penalty": -2.0}, {"repetition_penalty": 10.0}, {"repetition_penalty": 0.01},
        {"logit_bias": {str(i): 100 if i % 2 else -100 for i in range(300)}}, {"logit_bias": {}}, {"seed": 0}, {"top_k": 1}]


@pytest.mark.parametrize("fast_lane", [True, False])
async def test_validation_422(fast_lane):
    async def go(c):
        for bad in BAD:
            r = await c.post("/v1/chat/completions", json=dict(BODY, **bad))
            assert r.status_code == 422, (bad, r.status_code)
        for good in GOOD:
            r = await c.post("/v1/chat/completions", json=dict(BODY, **good))
            assert r.status_code == 200, (good, r.text)
    await _run(make(Recording(), fast_lane=fast_lane, cache={"enabled": False}), go)


async def test_native_backend_refuses_a_bias_outside_the_vocabulary_with_400():
    from vgate.backends.native import NativeBackend
    from vgate.runtime.engine import EngineConfig, LLMEngine
    be = NativeBackend.__new__(NativeBackend)
    be.engine = LLMEngine(EngineConfig(model="tiny", device="cpu", max_model_len=128, max_num_seqs=4,
                                       max_num_batched_tokens=64, num_kv_blocks=32, warmup=False))
    vocab = be.engine.arch.vocab_size
    be.engine.start()
    try:
        async def go(c):
            r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=3, logit_bias={str(vocab): 1.0}))
            assert r.status_code == 400 and "vocabulary" in r.json()["detail"], r.text
            r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=3, temperature=0.0,
                                                              logit_bias={str(vocab - 1): 100.0}))
            assert r.status_code == 200 and r.json()["usage"]["completion_tokens"] == 3, r.text
            be.engine.tp.size = 2  # processors under tensor parallelism: refused at admission
            try:
                r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=3, presence_penalty=0.5))
            finally:
                be.engine.tp.size = 1
            assert r.status_code == 400 and "tensor parallel" in r.json()["detail"], r.text
            r = await c.post("/v1/chat/completions", json=dict(BODY, max_tokens=2))
            assert r.status_code == 200
        await _run(make(be, cache={"enabled": False}), go)
    finally:
        be.engine.tp.size = 1
        be.engine.stop()
    assert be.engine.runner.proc_steps > 0


def test_engine_process_refuses_and_survives():
    """Engine core in its own process: a request it cannot serve is refused with ValueError before
    it crosses the pipe, and one that reaches the core anyway fails alone — the core keeps serving
    (penalised requests included, with the tokens of the in-process engine)."""
    import threading

    from vgate.runtime.engine import EngineConfig, LLMEngine
    from vgate.runtime.engine_process import EngineProcessClient
    from vgate.runtime.sampling_params import SamplingParams
    cfg = EngineConfig(model="tiny", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
                       num_kv_blocks=128, warmup=False, seed=0)
    prompt = [5 + (j * 11) % 400 for j in range(16)]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True, frequency_penalty=3.0,
                        logit_bias={t: 30.0 for t in (11, 57, 106)})
    ref = {}
    eng = LLMEngine(cfg)
    eng.add_request("r", prompt_ids=prompt, params=sp, callback=lambda k, s, p: ref.update(out=list(s.output_ids)))
    eng.run_until_idle()
    cli = EngineProcessClient(cfg)
    try:
        vocab = cli.snapshot()["vocab_size"]
        with pytest.raises(ValueError):
            cli.add_request("bad", prompt_ids=prompt, params=SamplingParams(logit_bias={vocab: 1.0}))
        # past the client's check (as a client without it would send it): the core rejects it alone
        from vgate.runtime.engine_process import SeqView
        raw = []
        cli._seqs["raw"] = (SeqView("raw"), lambda kind, seq, payload: raw.append((kind, payload)))
        cli._send(("add", "raw", None, prompt, SamplingParams(logit_bias={vocab + 7: 1.0}), False))
        res, ev = {}, threading.Event()

        def cb(kind, seq, payload):
            if kind != "token":
                res["ok"] = (kind, list(seq.output_ids))
                ev.set()
        cli.add_request("ok", prompt_ids=prompt, params=sp, callback=cb)
        assert ev.wait(120)
        assert res["ok"] == ("finish", ref["out"])
        assert len(raw) == 1 and raw[0][0] == "error" and "vocabulary" in raw[0][1], raw
        assert cli.healthy
    finally:
        cli.stop()
