"""Qwen3 (QK-norm) on the CPU: the reference op against a float64 formula, the config / presets, the dense
oracle against a float64 forward, the engine in its exact and bf16 modes, the checkpoint round trip and
TP = 2 over gloo. The GPU side is tests/test_qwen3_gpu.py."""
from __future__ import annotations

import dataclasses
import json

import pytest
import torch

import gemm_exact as X
import qwen3_cases as Q
from vgate import ops
from vgate.models.config import PRESETS, _from_hf_config, resolve_arch
from vgate.models.weights import QK_NORM_HI, QK_NORM_LO, save_checkpoint
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams


# ------------------------------------------------------------------ 1. the reference op
def _run_ref(c, dtype):
    T, Hq, Hkv = c["T"], c["Hq"], c["Hkv"]
    qkv = c["qkv"].to(dtype)
    before = qkv.clone()
    kc = torch.full((c["blocks"], Hkv, Q.BS, Q.D), X.SENT, dtype=dtype)
    vc = kc.clone()
    q_out = torch.full((T, Hq * Q.D + 40), X.SENT, dtype=dtype)
    ops.qk_norm_rope_kv(qkv, c["positions"], c["slots"], c["cos_sin"], c["q_norm"], c["k_norm"], Q.EPS, kc, vc, Hq, Hkv,
                        q_out)
    assert torch.equal(qkv, before), "qkv must not be modified"
    assert bool((q_out[:, Hq * Q.D:] == X.SENT).all())
    return q_out[:, : Hq * Q.D].reshape(T, Hq, Q.D), kc, vc


def test_reference_op_fp32_against_fp64_formula():
    c = Q.make_case(11, 3, 2, dtype=torch.float32)
    e = Q.expect64(c)
    q, kc, vc = _run_ref(c, torch.float32)
    assert bool((c["slots"] < 0).any()) and not torch.equal(c["q_norm"], c["k_norm"])
    # 1e-5 relative to the two products a c and b s whose sum or difference the element is (an element
    # that cancels to near zero keeps the products' absolute fp32 error)
    w = Q.written(c)
    Q.within(q, e["q"], 1e-5 * e["cancel_q"], "q fp32")
    Q.within(Q.cache_rows(kc, c), e["k"][w], 1e-5 * e["cancel_k"][w], "k cache fp32")
    unwritten = e["k_cache"] == X.SENT
    assert bool((kc.double()[unwritten] == X.SENT).all())
    assert torch.equal(vc.double(), e["v_cache"])


def test_reference_op_bf16_within_the_kernel_bound():
    """One rounding of n_a c -/+ n_b s: 2^-9 relative to the result, bounded through the cancellation by
    the two products, doubled (the bound of the GPU kernel test)."""
    c = Q.make_case(11, 3, 2)
    e = Q.expect64(c)
    q, kc, vc = _run_ref(c, torch.bfloat16)
    Q.within(q, e["q"], 2.0 ** -8 * e["cancel_q"], "q bf16")
    Q.within(Q.cache_rows(kc, c), e["k"][Q.written(c)], 2.0 ** -8 * e["cancel_k"][Q.written(c)], "k bf16")
    assert torch.equal(vc.double(), e["v_cache"])
    unwritten = e["k_cache"] == X.SENT
    assert bool(unwritten.any()) and bool((kc.double()[unwritten] == X.SENT).all())


# ------------------------------------------------------------------ 2. config
def test_hf_config_resolves_to_qwen3():
    cfg = dict(model_type="qwen3", head_dim=128, hidden_size=1024, num_attention_heads=16, num_key_value_heads=8,
               num_hidden_layers=28, intermediate_size=3072, vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1e6,
               tie_word_embeddings=True, max_position_embeddings=40960)
    a = _from_hf_config(cfg, "x")
    assert (a.family, a.qk_norm, a.qkv_bias, a.head_dim, a.q_size) == ("qwen3", True, False, 128, 2048)
    assert _from_hf_config(dict(cfg, attention_bias=True), "x").qkv_bias
    with pytest.raises(ValueError, match="qwen3_moe"):
        _from_hf_config(dict(cfg, model_type="qwen3_moe"), "x")
    # the other families resolve as before
    q2 = _from_hf_config(dict(cfg, model_type="qwen2"), "x")
    assert (q2.family, q2.qk_norm, q2.qkv_bias) == ("qwen2", False, True)
    ll = _from_hf_config(dict(cfg, model_type="llama"), "x")
    assert (ll.family, ll.qk_norm, ll.qkv_bias) == ("llama", False, False)


@pytest.mark.parametrize("model_id,preset,dims", [
    ("Qwen/Qwen3-0.6B", "qwen3-0.6b", (1024, 28, 16, 8, 128, 3072, True)),
    ("Qwen/Qwen3-1.7B", "qwen3-1.7b", (2048, 28, 16, 8, 128, 6144, True)),
    ("Qwen/Qwen3-4B", "qwen3-4b", (2560, 36, 32, 8, 128, 9728, True)),
    ("Qwen/Qwen3-8B", "qwen3-8b", (4096, 36, 32, 8, 128, 12288, False)),
])
def test_presets_and_aliases(model_id, preset, dims):
    a = resolve_arch(model_id)
    assert a is PRESETS[preset] and a.family == "qwen3" and a.qk_norm and not a.qkv_bias
    assert (a.hidden_size, a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim, a.intermediate_size,
            a.tie_embeddings) == dims
    assert (a.vocab_size, a.rms_eps, a.rope_theta, a.max_position, a.bos_token_id, a.eos_token_ids) == \
        (151936, 1e-6, 1e6, 40960, 151643, (151645, 151643))
    with_norm = a.num_params()
    assert with_norm - dataclasses.replace(a, qk_norm=False).num_params() == a.num_layers * 2 * a.head_dim


def test_existing_presets_unchanged():
    a = resolve_arch("Qwen/Qwen2.5-1.5B-Instruct")
    assert a is PRESETS["qwen2.5-1.5b"] and not a.qk_norm
    assert dataclasses.astuple(a)[:17] == ("qwen2.5-1.5b", "qwen2", 1536, 28, 12, 2, 128, 8960, 151936, 1e-6, 1e6, None,
                                           True, True, 32768, 151643, (151645, 151643))
    t = resolve_arch("tiny")
    assert t is PRESETS["tiny"] and not t.qk_norm
    assert dataclasses.astuple(t)[:17] == ("tiny", "qwen2", 256, 2, 4, 2, 128, 512, 512, 1e-6, 1e4, None, True, True,
                                           4096, 1, (2,))
    assert [f.name for f in dataclasses.fields(a)][-1] == "qk_norm"
    t3 = resolve_arch("tiny-qwen3")
    assert (t3.family, t3.qk_norm, t3.qkv_bias, t3.hidden_size, t3.num_layers, t3.num_heads, t3.num_kv_heads,
            t3.head_dim, t3.intermediate_size, t3.vocab_size, t3.tie_embeddings, t3.max_position) == \
        ("qwen3", True, False, 256, 2, 4, 2, 128, 512, 512, True, 4096)
    assert not any(p.qk_norm for k, p in PRESETS.items() if "qwen3" not in k)


# ------------------------------------------------------------------ engines (built once per module)
def _engine(**kw):
    cfg = dict(model="tiny-qwen3", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
               num_kv_blocks=64, warmup=False, seed=0)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _greedy(eng, n=12):
    done = {}

    def cb(kind, seq, payload):
        if kind in ("finish", "error"):
            done[seq.request_id] = list(seq.output_ids)

    sp = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)
    for k, v in Q.PROMPTS.items():
        eng.add_request(k, params=sp, callback=cb, prompt_ids=v)
    eng.run_until_idle()
    assert set(done) == set(Q.PROMPTS) and all(len(v) == n for v in done.values())
    return done


@pytest.fixture(scope="module")
def runs():
    """(engine, greedy tokens per prompt, teacher-forced reference rows per prompt) for both CPU modes."""
    out = {}
    for dt in ("float32", "bfloat16"):
        eng = _engine(dtype=dt)
        toks = _greedy(eng)
        rows = {k: eng.model.reference_logits(v + toks[k][:-1])[len(v) - 1:] for k, v in Q.PROMPTS.items()}
        out[dt] = (eng, toks, rows)
    return out


# ------------------------------------------------------------------ 3. the dense oracle
def _forward64(model, ids):
    """Dense float64 forward from the HF Qwen3 definition: RMSNorm, q / k / v projections, RMSNorm over
    each head's 128 dims with q_norm / k_norm, NeoX RoPE, causal softmax attention over repeated KV heads,
    o_proj, SwiGLU MLP, final norm, tied LM head."""
    a = model.arch
    n, Dh, eps = len(ids), a.head_dim, a.rms_eps
    G = a.num_heads // a.num_kv_heads

    def rms(t, w):
        return t / torch.sqrt((t * t).mean(-1, keepdim=True) + eps) * w.double()

    inv_freq = 1.0 / (a.rope_theta ** (torch.arange(0, Dh, 2, dtype=torch.float64) / Dh))
    ang = torch.outer(torch.arange(n, dtype=torch.float64), inv_freq)
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1)[:, None], torch.cat([ang.sin(), ang.sin()], -1)[:, None]

    def rot_half(t):
        return torch.cat([-t[..., Dh // 2:], t[..., : Dh // 2]], -1)

    h = model.embed[torch.tensor(ids)].double()
    for L in model.layers:
        x = rms(h, L.in_norm)
        w = L.qkv.dense_weight().double()
        assert L.qkv.bias is None
        q = (x @ w[: a.q_size].t()).view(n, a.num_heads, Dh)
        k = (x @ w[a.q_size: a.q_size + a.kv_size].t()).view(n, a.num_kv_heads, Dh)
        v = (x @ w[a.q_size + a.kv_size:].t()).view(n, a.num_kv_heads, Dh)
        q, k = rms(q, L.q_norm), rms(k, L.k_norm)
        q, k = q * cos + rot_half(q) * sin, k * cos + rot_half(k) * sin
        o = torch.empty(n, a.num_heads, Dh, dtype=torch.float64)
        for hd in range(a.num_heads):
            sc = q[:, hd] @ k[:, hd // G].t() / Dh ** 0.5
            sc = sc.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
            o[:, hd] = torch.softmax(sc, -1) @ v[:, hd // G]
        h = h + o.reshape(n, -1) @ L.o.dense_weight().double().t()
        x = rms(h, L.post_norm)
        gu = L.gate_up.dense_weight().double()
        I = gu.shape[0] // 2
        h = h + (torch.nn.functional.silu(x @ gu[:I].t()) * (x @ gu[I:].t())) @ L.down.dense_weight().double().t()
    return rms(h, model.final_norm) @ model.embed.double().t()


def test_reference_logits_against_fp64_forward(runs):
    model = runs["float32"][0].model
    ids = Q.PROMPTS["q0"] + [11, 400][: 9 - len(Q.PROMPTS["q0"])]
    assert len(ids) == 9
    got = model.reference_logits(ids).double()
    want = _forward64(model, ids)[:, : model.arch.vocab_size]
    assert float((got - want).abs().max()) <= 1e-3, float((got - want).abs().max())


# ------------------------------------------------------------------ 4. the CPU engine
def test_engine_fp32_tokens_are_the_reference_argmax(runs):
    _, toks, rows = runs["float32"]
    for k in Q.PROMPTS:
        assert toks[k] == [int(r.argmax()) for r in rows[k]], k


def test_engine_bf16_tokens_within_the_margin(runs):
    _, toks, rows = runs["bfloat16"]
    for k in Q.PROMPTS:
        for t, tok in enumerate(toks[k]):
            assert Q.margin_ok(rows[k][t], tok), (k, t)


# ------------------------------------------------------------------ 5. the fixture discriminates
def test_margin_fails_without_the_norm(runs):
    """With the norm weights replaced by ones, and then with the norm taken out of the oracle altogether,
    teacher-forced tokens of the real model miss the margin: a GPU path that dropped or misplaced the norm
    cannot pass the engine tests. random_init draws the weights uniform in [0.5, 4.0]."""
    assert (QK_NORM_LO, QK_NORM_HI) == (0.5, 4.0)
    eng, toks, _ = runs["bfloat16"]
    model = eng.model
    saved = [(L.q_norm, L.k_norm) for L in model.layers]
    arch = model.arch

    def failures():
        n = 0
        for k, v in Q.PROMPTS.items():
            rows = model.reference_logits(v + toks[k][:-1])[len(v) - 1:]
            n += sum(not Q.margin_ok(rows[t], tok) for t, tok in enumerate(toks[k]))
        return n

    try:
        for L in model.layers:
            assert float(L.q_norm.float().min()) >= 0.5 and float(L.q_norm.float().max()) <= 4.0
            assert float(L.q_norm.float().std()) > 0.5 and not torch.equal(L.q_norm, L.k_norm)
            L.q_norm, L.k_norm = torch.ones_like(L.q_norm), torch.ones_like(L.k_norm)
        ones = failures()
        model.arch = dataclasses.replace(arch, qk_norm=False)
        gone = failures()
    finally:
        model.arch = arch
        for L, (qn, kn) in zip(model.layers, saved):
            L.q_norm, L.k_norm = qn, kn
    assert ones >= 1 and gone >= 1, (ones, gone)
    assert failures() == 0


# ------------------------------------------------------------------ 6. checkpoint round trip
def test_checkpoint_round_trip(tmp_path, runs):
    from safetensors.torch import load_file, save_file
    eng, toks, _ = runs["bfloat16"]
    path = tmp_path / "ckpt"
    save_checkpoint(eng.model, str(path))
    cfg = json.loads((path / "config.json").read_text())
    assert cfg["model_type"] == "qwen3" and cfg["head_dim"] == 128
    back = resolve_arch(str(path))
    assert dataclasses.replace(back, name=eng.arch.name) == eng.arch and back.qk_norm
    loaded = _engine(model=str(path))
    assert all(L.qkv.layout == "plain" and L.q_norm is not None for L in loaded.model.layers)
    ids = Q.PROMPTS["q2"]
    assert torch.equal(loaded.model.reference_logits(ids), eng.model.reference_logits(ids))
    assert _greedy(loaded) == toks  # the saved directory serves the same tokens
    # a Qwen3 checkpoint without its q_norm tensors must not load
    tensors = load_file(str(path / "model.safetensors"))
    cut = {k: v for k, v in tensors.items() if ".q_norm." not in k}
    assert len(cut) == len(tensors) - eng.arch.num_layers
    bad = tmp_path / "bad"
    bad.mkdir()
    save_file(cut, str(bad / "model.safetensors"))
    (bad / "config.json").write_text((path / "config.json").read_text())
    with pytest.raises(ValueError, match="q_norm"):
        _engine(model=str(bad))


def test_weight_bytes_count_the_norms(runs):
    model = runs["bfloat16"][0].model
    with_norm = model.weight_bytes()
    saved = [(L.q_norm, L.k_norm) for L in model.layers]
    try:
        for L in model.layers:
            L.q_norm = L.k_norm = None
        assert with_norm - model.weight_bytes() == model.arch.num_layers * 2 * 128 * 2
    finally:
        for L, (qn, kn) in zip(model.layers, saved):
            L.q_norm, L.k_norm = qn, kn


# ------------------------------------------------------------------ 7. TP = 2 over gloo
@pytest.mark.timeout(300)
def test_tp2_matches_tp1(tmp_path):
    """The pattern of tests/test_tp_cpu.py: a TP = 2 engine loaded from the TP = 1 checkpoint (the two norm
    weights replicated, the plain-layout QKV rows sharded by head) generates the TP = 1 tokens."""
    import test_tp_cpu as TP
    base = LLMEngine(EngineConfig(model="tiny-qwen3", device="cpu", max_model_len=256, max_num_seqs=8,
                                  max_num_batched_tokens=64, num_kv_blocks=128, warmup=False, seed=0))
    path = str(tmp_path / "ckpt")
    save_checkpoint(base.model, path)
    ref_eng = LLMEngine(TP._cfg(path, 1))
    assert ref_eng.arch.qk_norm
    ref = TP._generate(ref_eng)
    assert set(ref) == set(TP.PROMPTS) and all(len(v) == 8 for v in ref.values())
    assert TP._run_group(2, path) == ref
