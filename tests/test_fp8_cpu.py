"""FP8 (e4m3 W8A16) without a GPU: the integer problems of tests/fp8_cases.py, packing, load-time
quantization, the checkpoint loader's three scale forms, the config switch and the CPU engine (TP 1 and 2).
The GPU kernels are checked by tests/test_fp8_gpu.py against the same ``Linear.dense_weight()``."""
from __future__ import annotations

import json

import pytest
import torch
import torch.multiprocessing as mp
from safetensors.torch import load_file, save_file

import fp8_cases as F
import test_tp_cpu as T
from vgate import ops
from vgate.config import VGateConfig
from vgate.models.config import resolve_arch
from vgate.models.transformer import DecoderModel
from vgate.models.weights import save_checkpoint
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams

FP8 = torch.float8_e4m3fn
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
        "mlp.up_proj", "mlp.down_proj")


# ------------------------------------------------------------------ problems, packing, quantization
def test_every_registered_problem_meets_its_preconditions():
    assert len(F.SPECS) > 50
    for s in sorted(F.SPECS, key=str):
        p = F.build(s)  # Problem.check: integral, within BOUND, codes x scales == w
        lin = ops.Linear(None, p.bias, fp8=dict(p.fp8, layout=p.kind))
        assert lin.kind == "fp8" and torch.equal(lin.dense_weight(), p.w), s


def test_perturb_moves_one_column():
    p = F.build(F.spec_for("bias", 8, 256, 512, "block"))
    pp = F.perturb(p, 255, 300)
    d = (pp.w.double() != p.w.double()).nonzero().tolist()
    assert d == [[255, 300]]
    assert float(pp.fp8["codes"].view(FP8)[255, 300]) in (2.0, 3.0)
    assert int((pp.fp8["codes"] != p.fp8["codes"]).sum()) == 1


@pytest.mark.parametrize("N,K", [(16, 128), (F.ODD_N, 1536)])
def test_pack_fp8_round_trip_and_layout(N, K):
    g = torch.Generator().manual_seed(N + K)
    c = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    pk = ops.pack_fp8(c)
    assert pk.shape == (N // 16, K // 64, 64, 16) and pk.is_contiguous()
    assert torch.equal(ops.unpack_fp8(pk, N, K), c)
    for nt, kp, lane, u, j in torch.randint(0, 1 << 20, (500, 5), generator=g).tolist():
        nt, kp, lane, u, j = nt % (N // 16), kp % (K // 64), lane % 64, u % 2, j % 8
        assert pk[nt, kp, lane, 8 * u + j] == c[16 * nt + (lane & 15), 64 * kp + 32 * u + 8 * (lane >> 4) + j]


def test_linear_fp8_rejects_bad_shapes():
    c = torch.zeros(16, 192, dtype=torch.uint8)
    with pytest.raises(ValueError, match="K % 128"):
        ops.Linear(None, fp8=dict(codes=c, scales=torch.ones(1, 16)))
    with pytest.raises(ValueError, match="scales"):
        ops.Linear(None, fp8=dict(codes=torch.zeros(16, 256, dtype=torch.uint8), scales=torch.ones(3, 16)))


def test_gemm_route_of_an_fp8_linear():
    """M <= 16: the fp8 decode kernel with the Linear's decode knobs; M > 16: dequant + the bf16 kernels on the
    Linear's prefill plan; row gather, fused all-reduce and the norm hand-off raise."""
    p = F.build(F.spec_for("bias", 8, 256, 512, "channel"))
    lin = ops.Linear(None, fp8=dict(p.fp8))
    kw = dict(waves=0, splitk=0, path=0, row_idx=None, ar=None, norm_out=None)
    assert ops._gemm_route(lin, 16, **kw) == ("gemm", ops.PATH_AUTO, 0, 0, 0)
    lin.dec_waves, lin.dec_splitk, lin.dec_ntb = 4, 2, 2
    assert ops._gemm_route(lin, 1, **kw) == ("gemm", ops.PATH_AUTO, 4, 2, 2)
    assert ops._gemm_route(lin, 8, **dict(kw, waves=2, splitk=3)) == ("gemm", ops.PATH_AUTO, 2, 3, 0)
    assert ops._gemm_route(lin, 17, **kw) == ("dequant", {})
    lin.prefill_plan = {448: (128, 2)}
    assert ops._gemm_route(lin, 300, **kw) == ("dequant", ops._plan_kw((128, 2), 300))
    for bad in (dict(row_idx=torch.zeros(2, dtype=torch.int32)), dict(ar=object()), dict(norm_out=(None, None, None))):
        with pytest.raises(ValueError, match="fp8 Linear"):
            ops._gemm_route(lin, 8, **dict(kw, **bad))
    assert not lin.fold_norm(torch.ones(512))


def test_quantize_fp8_error_bound_and_zero_row():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(96, 384, generator=g) * torch.logspace(-3, 1, 96)[:, None]).bfloat16()
    w[7] = 0
    lin = ops.Linear.quantize_fp8(w, layout="plain")
    assert lin.kind == "fp8" and lin.N == 96 and lin.K == 384
    d = lin.dense_weight()
    assert d.dtype == torch.bfloat16 and bool(torch.isfinite(d).all())
    assert bool((d[7] == 0).all())
    # e4m3 has 3 mantissa bits: half an ulp is at most 2^-4 of |w| for normal codes (1/17 at the worst
    # midpoint, which leaves room for bf16's rounding of code * s); below the smallest normal (2^-6 s) the
    # step is the subnormal one, 2^-9 s, the row's smallest step, s = amax_row / 448
    wf = w.float()
    s = torch.where(wf.abs().amax(1) > 0, wf.abs().amax(1) / 448, torch.ones(96))
    tol = 2.0 ** -4 * wf.abs() + (2.0 ** -9 * s)[:, None]
    assert bool(((d.float() - wf).abs() <= tol).all())
    assert lin.nbytes() == 96 * 384 * 2  # CPU Linear keeps the bf16 matrix


def test_config_accepts_fp8(monkeypatch):
    for k in list(__import__("os").environ):
        if k.startswith("VGATE_"):
            monkeypatch.delenv(k)
    assert VGateConfig(model={"quantization": "fp8"}).model.quantization == "fp8"
    assert VGateConfig(model={"quantization": "FP8"}).model.quantization == "fp8"
    with pytest.raises(Exception, match="awq, fp8"):
        VGateConfig(model={"quantization": "gptq"})


# ------------------------------------------------------------------ checkpoints
def _block_quant(w: torch.Tensor):
    """128 x 128 block scales: (codes fp8 [N, K], scale_inv fp32 [ceil(N/128), ceil(K/128)], expanded [N, K])."""
    N, K = w.shape
    nb, kb = (N + 127) // 128, (K + 127) // 128
    wf = torch.zeros(nb * 128, kb * 128)
    wf[:N, :K] = w.float()
    amax = wf.reshape(nb, 128, kb, 128).abs().amax(dim=(1, 3))
    s = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    full = s.repeat_interleave(128, 0).repeat_interleave(128, 1)[:N, :K]
    return (w.float() / full).clamp(-448, 448).to(FP8), s, full


def _row_quant(w: torch.Tensor, per_tensor: bool):
    wf = w.float()
    amax = wf.abs().amax() if per_tensor else wf.abs().amax(1, keepdim=True)
    s = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    return (wf / s).clamp(-448, 448).to(FP8), s, s.expand_as(wf)


@pytest.fixture(scope="module")
def dense_ckpt(tmp_path_factory):
    """A bf16 checkpoint of the 2-layer 'tiny' preset (128-wide heads) and its tensors."""
    path = tmp_path_factory.mktemp("fp8") / "bf16"
    model = DecoderModel(resolve_arch("tiny"), "cpu", seed=3)
    save_checkpoint(model, str(path))
    return path, load_file(str(path / "model.safetensors"))


def _write_fp8(dense_ckpt, dst, form: str, mutate=None, cfg_extra=None):
    """The checkpoint with every projection as e4m3 codes + scales; returns {weight name: bf16(code * scale)}."""
    src, tensors = dense_ckpt
    out, want = {}, {}
    for name, t in tensors.items():
        if not (name.endswith(".weight") and any(p in name for p in PROJ)):
            out[name] = t
            continue
        base = name[: -len(".weight")]
        if form == "block":
            codes, s, full = _block_quant(t)
            out[base + ".weight_scale_inv"] = s
        else:
            codes, s, full = _row_quant(t, form.startswith("tensor"))
            shape = {"channel": (-1, 1), "channel_flat": (-1,), "tensor": (), "tensor_1": (1,)}[form]
            out[base + ".weight_scale"] = s.reshape(shape)
            out[base + ".input_scale"] = torch.tensor(0.5)  # activation scale: ignored (W8A16)
        out[name] = codes
        want[name] = (codes.float() * full).to(torch.bfloat16)
    if mutate:
        mutate(out)
    dst.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in out.items()}, str(dst / "model.safetensors"))
    cfg = json.loads((src / "config.json").read_text())
    cfg["quantization_config"] = {"quant_method": "fp8", "fmt": "e4m3"}
    if form == "block":
        cfg["quantization_config"]["weight_block_size"] = [128, 128]
    cfg["quantization_config"].update(cfg_extra or {})
    (dst / "config.json").write_text(json.dumps(cfg))
    return want


def _expect_layers(model, want):
    for i, L in enumerate(model.layers):
        p = f"model.layers.{i}."
        qkv = torch.cat([want[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        gu = torch.cat([want[p + "mlp.gate_proj.weight"], want[p + "mlp.up_proj.weight"]])
        for lin, w in ((L.qkv, qkv), (L.o, want[p + "self_attn.o_proj.weight"]), (L.gate_up, gu),
                       (L.down, want[p + "mlp.down_proj.weight"])):
            assert lin.kind == "fp8"
            assert torch.equal(lin.dense_weight(), w), (i, lin.layout)
        assert L.qkv.bias is not None and L.qkv.layout == "qkv" and L.gate_up.layout == "silu"
    assert model.lm_head.kind == "dense"


@pytest.mark.parametrize("form", ["block", "channel", "channel_flat", "tensor", "tensor_1"])
def test_loader_reads_every_scale_form(dense_ckpt, tmp_path, form):
    want = _write_fp8(dense_ckpt, tmp_path / form, form)
    model = DecoderModel(resolve_arch(str(tmp_path / form)), "cpu", weights_path=str(tmp_path / form))
    _expect_layers(model, want)


def test_loader_quantizes_a_bf16_checkpoint_at_load(dense_ckpt):
    src, tensors = dense_ckpt
    model = DecoderModel(resolve_arch(str(src)), "cpu", weights_path=str(src), quantization="fp8")
    want = {k: ops.Linear.quantize_fp8(v).dense_weight() for k, v in tensors.items()
            if k.endswith(("o_proj.weight", "down_proj.weight"))}
    for i, L in enumerate(model.layers):
        p = f"model.layers.{i}."
        assert all(lin.kind == "fp8" for lin in (L.qkv, L.o, L.gate_up, L.down))
        assert torch.equal(L.o.dense_weight(), want[p + "self_attn.o_proj.weight"])
        assert torch.equal(L.down.dense_weight(), want[p + "mlp.down_proj.weight"])
        qkv = torch.cat([tensors[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        assert torch.equal(L.qkv.dense_weight(), ops.Linear.quantize_fp8(qkv).dense_weight())
    dense = DecoderModel(resolve_arch(str(src)), "cpu", weights_path=str(src))
    assert all(L.qkv.kind == "dense" for L in dense.layers)


def _as(dtype):
    def mutate(out):
        k = "model.layers.1.mlp.down_proj.weight"
        out[k] = out[k].float().to(dtype)
    return mutate


def _drop_scale(out):
    del out["model.layers.0.self_attn.o_proj.weight_scale_inv"]


@pytest.mark.parametrize("form,mutate,cfg_extra,match", [
    ("block", _as(torch.float8_e5m2), None, "float8_e5m2"),
    ("block", _as(torch.float8_e4m3fnuz), None, "float8_e4m3fnuz"),
    ("block", _drop_scale, None, "without weight_scale"),
    ("block", None, {"weight_block_size": [64, 64]}, "weight_block_size"),
    ("block", None, {"weight_block_size": None}, "weight_block_size"),
], ids=["e5m2", "e4m3fnuz", "no_scale", "block_64", "no_block_size"])
def test_loader_rejects(dense_ckpt, tmp_path, form, mutate, cfg_extra, match):
    _write_fp8(dense_ckpt, tmp_path / "bad", form, mutate, cfg_extra)
    with pytest.raises(ValueError, match=match):
        DecoderModel(resolve_arch(str(tmp_path / "bad")), "cpu", weights_path=str(tmp_path / "bad"))


def test_loader_rejects_a_float8_embedding(dense_ckpt, tmp_path):
    def mutate(out):
        out["model.norm.weight"] = out["model.norm.weight"].float().to(FP8)
    _write_fp8(dense_ckpt, tmp_path / "bad", "channel", mutate)
    with pytest.raises(ValueError, match="model.norm.weight"):
        DecoderModel(resolve_arch(str(tmp_path / "bad")), "cpu", weights_path=str(tmp_path / "bad"))


# ------------------------------------------------------------------ engines
def _greedy(eng, prompts, n=10):
    done = {}

    def cb(kind, seq, payload):
        if kind in ("finish", "error"):
            done[seq.request_id] = list(seq.output_ids)

    sp = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)
    for k, v in prompts.items():
        eng.add_request(k, params=sp, callback=cb, prompt_ids=v)
    eng.run_until_idle()
    assert set(done) == set(prompts) and all(len(v) == n for v in done.values())
    return done


def test_cpu_engine_fp8_tokens_are_the_reference_argmax():
    """random_init under quantization='fp8': the dense branch's draws, quantized per channel; the exact CPU
    mode's greedy tokens are the argmax of the fp32 forward on the dequantised weights, teacher-forced."""
    cfg = dict(model="tiny", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
               num_kv_blocks=64, warmup=False, seed=0, dtype="float32")
    eng = LLMEngine(EngineConfig(quantization="fp8", **cfg))
    dense = LLMEngine(EngineConfig(**cfg))
    for Lq, Ld in zip(eng.model.layers, dense.model.layers):
        for a in ("qkv", "o", "gate_up", "down"):
            lq, ld = getattr(Lq, a), getattr(Ld, a)
            assert lq.kind == "fp8" and ld.kind == "dense" and lq.layout == ld.layout
            assert torch.equal(lq.dense_weight(), ops.Linear.quantize_fp8(ld.dense_weight()).dense_weight())
    assert eng.model.lm_head.kind == "dense" and torch.equal(eng.model.embed, dense.model.embed)
    toks = _greedy(eng, T.PROMPTS)
    for k, v in T.PROMPTS.items():
        rows = eng.model.reference_logits(v + toks[k][:-1])[len(v) - 1:]
        assert toks[k] == [int(r.argmax()) for r in rows], k


def _tp_worker(rank, world, port, path, q):
    """One gloo rank in the exact CPU mode (fp32 activations: the ranks' partial sums are not rounded to
    bf16 before the all-reduce, so TP = 2 and TP = 1 differ by fp32 summation order only)."""
    import os
    import traceback
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        torch.set_num_threads(1)
        eng = LLMEngine(T._cfg(path, world, dtype="float32"))
        assert eng.tp.size == world and eng.tp.rank == rank
        assert all(lin.kind == "fp8" for L in eng.model.layers for lin in (L.qkv, L.o, L.gate_up, L.down))
        if rank == 0:
            out = T._generate(eng)
            eng.shutdown_followers()
            q.put(("ok", out))
        else:
            eng.follower_loop()
            q.put(("ok", None))
    except Exception:  # noqa: BLE001
        q.put(("err", traceback.format_exc()))


@pytest.mark.timeout(300)
def test_tp2_fp8_matches_tp1(dense_ckpt, tmp_path):
    """A block-scaled FP8 checkpoint sharded over two gloo ranks (rows of qkv / gate_up, 128-multiple
    k-ranges of o / down with their scale blocks) generates the TP = 1 engine's tokens, and every rank's
    matrices are the slices of the TP = 1 ones."""
    from vgate.parallel.comm import TPGroup
    path = tmp_path / "ckpt"
    _write_fp8(dense_ckpt, path, "block")
    e1 = LLMEngine(T._cfg(str(path), 1, dtype="float32"))
    a = e1.arch
    for r in range(2):
        sh = DecoderModel(a, "cpu", tp=TPGroup(rank=r, size=2, simulated=True), weights_path=str(path))
        hq, hkv, I = a.q_size // 2, a.kv_size // 2, a.intermediate_size // 2
        for Lf, Ls in zip(e1.model.layers, sh.layers):
            w = Lf.qkv.dense_weight()
            q_, k_, v_ = w[: a.q_size], w[a.q_size: a.q_size + a.kv_size], w[a.q_size + a.kv_size:]
            assert torch.equal(Ls.qkv.dense_weight(), torch.cat([q_[r * hq: (r + 1) * hq], k_[r * hkv: (r + 1) * hkv],
                                                                 v_[r * hkv: (r + 1) * hkv]]))
            gu = Lf.gate_up.dense_weight()
            assert torch.equal(Ls.gate_up.dense_weight(), torch.cat([gu[: 2 * I][r * I: (r + 1) * I],
                                                                     gu[2 * I:][r * I: (r + 1) * I]]))
            assert torch.equal(Ls.o.dense_weight(), Lf.o.dense_weight()[:, r * hq: (r + 1) * hq])
            assert torch.equal(Ls.down.dense_weight(), Lf.down.dense_weight()[:, r * I: (r + 1) * I])
    assert all(L.down.kind == "fp8" for L in e1.model.layers)
    ref = T._generate(e1)
    assert set(ref) == set(T.PROMPTS) and all(len(v) == 8 for v in ref.values())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = T._free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, str(path), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    errs = [r[1] for r in results if r[0] == "err"]
    assert not errs, errs[0]
    assert next(r[1] for r in results if r[1] is not None) == ref
