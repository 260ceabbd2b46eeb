"""MXFP4 (e2m1 W4A16, e8m0 block-32 scales) without a GPU: the integer problems of tests/mxfp4_cases.py,
packing, OCP MX quantization against a float64 oracle written here, every scale / shape / dtype rejection, the
checkpoint loader (TP 1 and 2), the config switch, the route, the CPU engine and the chat API.
The GPU kernels are checked by tests/test_mxfp4_gpu.py against the same ``Linear.dense_weight()``."""
from __future__ import annotations

import json

import httpx
import pytest
import torch
import torch.multiprocessing as mp
from safetensors.torch import load_file, save_file

import mxfp4_cases as F
import test_tp_cpu as T
from vgate import ops
from vgate.api.app import create_app
from vgate.backends.native import NativeBackend
from vgate.config import VGateConfig
from vgate.engine import VGateEngine
from vgate.models.config import resolve_arch
from vgate.models.transformer import DecoderModel
from vgate.models.weights import save_checkpoint
from vgate.ops import packing
from vgate.runtime.engine import EngineConfig, LLMEngine
from vgate.runtime.sampling_params import SamplingParams

PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
        "mlp.up_proj", "mlp.down_proj")
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


# ------------------------------------------------------------------ problems, packing
def test_every_registered_problem_meets_its_preconditions():
    assert len(F.SPECS) > 50
    for s in sorted(F.SPECS, key=str):
        p = F.build(s)  # Problem.check: integral, within BOUND, codes x scales == w
        lin = ops.Linear(None, p.bias, mxfp4=dict(p.mxfp4, layout=p.kind))
        assert lin.kind == "mxfp4" and torch.equal(lin.dense_weight(), p.w), s
        assert len(set(p.mxfp4["scales"].flatten().tolist())) == 3 or p.kind == "silu"


def test_perturbations_move_one_column():
    p = F.build(F.spec_for("bias", 8, 256, 512))
    pp = F.perturb(p, 255, 300)
    assert (pp.w.double() != p.w.double()).nonzero().tolist() == [[255, 300]]
    assert int((pp.mxfp4["codes"] != p.mxfp4["codes"]).sum()) == 1 and int(pp.mxfp4["codes"][255, 300]) in (4, 6)
    n, kb = F.active_block(p, 17)
    ps = F.perturb_scale(p, n, kb)
    assert int((ps.mxfp4["scales"] != p.mxfp4["scales"]).sum()) == 1 and torch.equal(ps.mxfp4["codes"], p.mxfp4["codes"])
    d = (ps.w.double() != p.w.double()).nonzero()
    assert len(d) >= 1 and set(d[:, 0].tolist()) == {n} and all(kb * 32 <= k < kb * 32 + 32 for k in d[:, 1].tolist())
    cols = (ps.exp["biased"] != p.exp["biased"]).nonzero()[:, 1].tolist()
    assert cols and set(cols) == {n}


def test_every_code_table_is_what_it_says():
    codes, scales, x, km = F.every_code_table()
    assert sorted(set((km // 32).tolist())) == list(range(16))  # 16 distinct blocks of K = 512
    assert {2, 126, 127, 128, 252} <= set(F.EVERY_CODE_SCALES) and min(F.EVERY_CODE_SCALES) == 2
    assert max(F.EVERY_CODE_SCALES) == 252
    lin = ops.Linear(None, mxfp4=dict(codes=codes, scales=scales))
    out = x.double() @ lin.dense_weight().double().t()  # [m][n]
    want = F.every_code_values()
    assert torch.equal(out, want)
    assert float(want[0, 1]) == 2.0 ** -126 and float(want[15, 7]) == 6 * 2.0 ** 125 and float(want[6, 13]) == -3.0


@pytest.mark.parametrize("N,K", [(16, 128), (F.ODD_N, 1536)])
def test_pack_round_trips_and_layout(N, K):
    g = torch.Generator().manual_seed(N + K)
    c = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    s = torch.randint(0, 256, (N, K // 32), generator=g, dtype=torch.uint8)
    pk, ps = ops.pack_mxfp4(c), ops.pack_mxfp4_scales(s)
    assert pk.shape == (N // 16, K // 128, 64, 16) and pk.is_contiguous() and pk.dtype == torch.uint8
    assert ps.shape == (N // 16, K // 128, 16, 4) and ps.is_contiguous() and ps.dtype == torch.uint8
    assert torch.equal(ops.unpack_mxfp4(pk, N, K), c) and torch.equal(ops.unpack_mxfp4_scales(ps, N, K), s)
    for nt, kq, lane, u, j in torch.randint(0, 1 << 20, (500, 5), generator=g).tolist():
        nt, kq, lane, u, j = nt % (N // 16), kq % (K // 128), lane % 64, u % 4, j % 8
        dword = int.from_bytes(bytes(pk[nt, kq, lane, 4 * u: 4 * u + 4].tolist()), "little")
        n, k = 16 * nt + (lane & 15), 128 * kq + 32 * u + 8 * (lane >> 4) + j
        assert (dword >> (4 * j)) & 0xF == int(c[n, k])
        assert int(ps[nt, kq, lane & 15, u]) == int(s[n, k // 32])  # the lane's dword u: one scale block


# ------------------------------------------------------------------ quantization against a float64 oracle
def _oracle(w: torch.Tensor):
    """OCP MX v1.0, element by element in Python floats: per 32-block e = floor(log2(amax)) - 2 + 127 (127 for a
    zero block); each element / 2^(e-127) goes to the nearest of the 8 magnitudes, a tie to the one with an
    even mantissa bit (0, 1, 2, 4: even; 0.5, 1.5, 3, 6: odd), beyond 6 to 6. Returns (dequantised float64, e)."""
    import math
    N, K = w.shape
    grid = GRID.tolist()
    even = [True, False, True, False, True, False, True, False]
    out = torch.zeros(N, K, dtype=torch.float64)
    es = torch.zeros(N, K // 32, dtype=torch.long)
    for n in range(N):
        for b in range(K // 32):
            blk = [float(v) for v in w[n, 32 * b: 32 * b + 32].double()]
            amax = max(abs(v) for v in blk)
            e = 127 if amax == 0 else math.frexp(amax)[1] - 1 - 2 + 127
            es[n, b] = e
            s = 2.0 ** (e - 127)
            for i, v in enumerate(blk):
                a = abs(v) / s
                best = None
                for gi, gv in enumerate(grid):
                    d = abs(a - gv)
                    if best is None or d < best[0] or (d == best[0] and even[gi]):
                        best = (d, gi)
                q = grid[best[1]]
                out[n, 32 * b + i] = math.copysign(q * s, v)
    return out, es


def test_quantize_mxfp4_against_the_oracle():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(16, 256, generator=g) * torch.logspace(-3, 2, 16)[:, None]).bfloat16()
    w[3, 64:96] = 0                                   # a zero block
    w[4, 0:32] = w[4, 0:32].clamp(-3.0, 3.0) * 0.25
    w[4, 5] = 6 * 2.0 ** -2                           # amax exactly 6 * 2^k
    w[5, 32:64] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0,
                                4.0, -6.0] * 2).bfloat16()  # exact ties under scale 1 (amax 6)
    w[6, 96:128] = torch.tensor([7.0, -7.5, 7.75, 6.5, -7.0] + [0.1] * 27).bfloat16()  # amax in [4, 8): e = 127; > 6 saturates
    lin = ops.Linear.quantize_mxfp4(w)
    assert lin.kind == "mxfp4" and (lin.N, lin.K) == (16, 256)
    codes, scales = packing.mxfp4_quantize(w)
    want, es = _oracle(w)
    assert torch.equal(scales.long(), es)
    assert int(scales[3, 2]) == 127 and int(scales[4, 0]) == 127 - 2 and int(scales[5, 1]) == 127
    d = lin.dense_weight()
    assert d.dtype == torch.bfloat16 and torch.equal(d.double(), want)
    assert bool((d[3, 64:96] == 0).all())
    assert d[5, 32:46].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert d[6, 96:101].tolist() == [6.0, -6.0, 6.0, 6.0, -6.0]
    assert float(d[4, 5]) == 1.5
    assert lin.nbytes() == 16 * 256 * 2  # a CPU Linear keeps the bf16 matrix
    # with s = 2^(e-127): an element up to 6 s is within half the widest grid step (6 - 4) / 2 = 1 s of its
    # value; the block's amax is below 8 s, so an element beyond 6 s saturates with an error below 2 s
    err, a = (d.double() - w.double()).abs(), w.double().abs()
    s = torch.exp2(es.double() - 127).repeat_interleave(32, dim=1)
    assert bool((a < 8 * s).all()) and bool((err <= torch.where(a <= 6 * s, s, 2 * s)).all())


# ------------------------------------------------------------------ rejections
def _lin(codes, scales):
    return ops.Linear(None, mxfp4=dict(codes=codes, scales=scales))


def test_linear_mxfp4_rejects_bad_operands_and_scale_bytes():
    ok_c = torch.full((16, 128), 2, dtype=torch.uint8)
    ok_s = torch.full((16, 4), 127, dtype=torch.uint8)
    assert _lin(ok_c, ok_s).kind == "mxfp4"
    with pytest.raises(ValueError, match="K % 128"):
        _lin(torch.zeros(16, 192, dtype=torch.uint8), torch.full((16, 6), 127, dtype=torch.uint8))
    with pytest.raises(ValueError, match="N % 16"):
        _lin(torch.zeros(8, 128, dtype=torch.uint8), torch.full((8, 4), 127, dtype=torch.uint8))
    with pytest.raises(ValueError, match="codes"):
        _lin(ok_c.to(torch.int32), ok_s)
    with pytest.raises(ValueError, match="0..15"):
        _lin(ok_c + 20, ok_s)
    with pytest.raises(ValueError, match="scales"):
        _lin(ok_c, torch.full((16, 3), 127, dtype=torch.uint8))
    with pytest.raises(ValueError, match="scales"):
        _lin(ok_c, ok_s.float())
    for byte in (0, 1, 253, 254):  # outside 2..252 on a non-zero block
        s = ok_s.clone()
        s[5, 2] = byte
        with pytest.raises(ValueError, match=f"scale byte {byte}"):
            _lin(ok_c, s)
    for byte in (2, 252):
        s = ok_s.clone()
        s[5, 2] = byte
        assert bool(torch.isfinite(_lin(ok_c, s).dense_weight()).all())
    s = ok_s.clone()
    s[5, 2] = 255
    with pytest.raises(ValueError, match="255"):
        _lin(ok_c, s)
    # an all-zero block (codes +0 / -0) may carry any byte but 255: rewritten to 127
    c = ok_c.clone()
    c[5, 64:96] = torch.tensor([0, 8] * 16, dtype=torch.uint8)
    for byte in (0, 1, 200, 254):
        s = ok_s.clone()
        s[5, 2] = byte
        lin = _lin(c, s)
        assert bool((lin.dense_weight()[5, 64:96] == 0).all())
        assert torch.equal(packing.mxfp4_check_scales(c, s, "t"), ok_s)
    s[5, 2] = 255
    with pytest.raises(ValueError, match="255"):
        _lin(c, s)


def test_gemm_route_of_an_mxfp4_linear():
    """M <= 16: the mxfp4 decode kernel with the Linear's decode knobs; M > 16: dequant + the bf16 kernels on
    the Linear's prefill plan; row gather, fused all-reduce and the norm hand-off raise."""
    p = F.build(F.spec_for("bias", 8, 256, 512))
    lin = ops.Linear(None, mxfp4=dict(p.mxfp4))
    kw = dict(waves=0, splitk=0, path=0, row_idx=None, ar=None, norm_out=None)
    assert ops._gemm_route(lin, 1, **kw) == ("gemm", ops.PATH_AUTO, 0, 0, 0)
    assert ops._gemm_route(lin, 16, **kw) == ("gemm", ops.PATH_AUTO, 0, 0, 0)
    lin.dec_waves, lin.dec_splitk, lin.dec_ntb = 4, 2, 4
    assert ops._gemm_route(lin, 1, **kw) == ("gemm", ops.PATH_AUTO, 4, 2, 4)
    assert ops._gemm_route(lin, 16, **kw) == ("gemm", ops.PATH_AUTO, 4, 2, 4)
    assert ops._gemm_route(lin, 8, **dict(kw, waves=2, splitk=3)) == ("gemm", ops.PATH_AUTO, 2, 3, 0)
    assert ops._gemm_route(lin, 17, **kw) == ("dequant", {})
    assert ops._gemm_route(lin, 64, **kw) == ("dequant", {})
    lin.prefill_plan = {448: (128, 2)}
    assert ops._gemm_route(lin, 300, **kw) == ("dequant", ops._plan_kw((128, 2), 300))
    for bad in (dict(row_idx=torch.zeros(2, dtype=torch.int32)), dict(ar=object()), dict(norm_out=(None, None, None))):
        with pytest.raises(ValueError, match="mxfp4 Linear"):
            ops._gemm_route(lin, 8, **dict(kw, **bad))
    assert not lin.fold_norm(torch.ones(512))


def test_custom_allreduce_never_fuses_an_mxfp4_linear():
    from vgate.parallel.custom_allreduce import CustomAllReduce
    ar = CustomAllReduce.__new__(CustomAllReduce)
    ar.fused, ar.device = True, torch.device("cpu")
    x, out = torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(4, 16, dtype=torch.bfloat16)
    lin = _lin(torch.full((16, 128), 2, dtype=torch.uint8), torch.full((16, 4), 127, dtype=torch.uint8))
    assert ar.fuses(ops.Linear(torch.zeros(16, 128, dtype=torch.bfloat16)), x, out) and not ar.fuses(lin, x, out)


def test_config_accepts_mxfp4(monkeypatch):
    for k in list(__import__("os").environ):
        if k.startswith("VGATE_"):
            monkeypatch.delenv(k)
    assert VGateConfig(model={"quantization": "mxfp4"}).model.quantization == "mxfp4"
    assert VGateConfig(model={"quantization": "MXFP4"}).model.quantization == "mxfp4"
    assert VGateConfig(model={"quantization": "fp8"}).model.quantization == "fp8"
    with pytest.raises(Exception, match="awq, fp8, mxfp4"):
        VGateConfig(model={"quantization": "gptq"})


# ------------------------------------------------------------------ checkpoints
@pytest.fixture(scope="module")
def dense_ckpt(tmp_path_factory):
    """A bf16 checkpoint of the 2-layer 'tiny' preset (128-wide heads) and its tensors."""
    path = tmp_path_factory.mktemp("mxfp4") / "bf16"
    model = DecoderModel(resolve_arch("tiny"), "cpu", seed=3)
    save_checkpoint(model, str(path))
    return path, load_file(str(path / "model.safetensors"))


def _oracle_fast(w: torch.Tensor):
    """The oracle's rule vectorised in float64 with an explicit nearest-of-8 search (ties to the even
    entries), independent of packing.mxfp4_quantize's rounding arithmetic: (codes, scales, dequantised)."""
    N, K = w.shape
    x = w.double().reshape(N, K // 32, 32)
    amax = x.abs().amax(2)
    e = torch.where(amax > 0, torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))) + 125,
                    torch.full_like(amax, 127.0))
    a = x.abs() / torch.exp2(e - 127)[..., None]
    d = (a[..., None] - GRID).abs()
    d = d - torch.tensor([1e-12, 0, 1e-12, 0, 1e-12, 0, 1e-12, 0], dtype=torch.float64)  # a tie goes to the even entry
    idx = d.argmin(-1)
    codes = (idx | (torch.signbit(x).long() << 3)).to(torch.uint8).reshape(N, K)
    deq = (torch.where(torch.signbit(x), -1.0, 1.0) * GRID[idx] * torch.exp2(e - 127)[..., None]).reshape(N, K)
    return codes, e.to(torch.uint8), deq


def _write_mxfp4(dense_ckpt, dst, mutate=None):
    """The checkpoint with every projection as <proj>.weight uint8 [N, K/2] (element 2i in the low nibble) +
    <proj>.weight_scale uint8 [N, K/32]; returns {weight name: the oracle's dequantised bf16}."""
    src, tensors = dense_ckpt
    out, want = {}, {}
    for name, t in tensors.items():
        if not (name.endswith(".weight") and any(p in name for p in PROJ)):
            out[name] = t
            continue
        base = name[: -len(".weight")]
        codes, scales, deq = _oracle_fast(t)
        out[name] = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
        out[base + ".weight_scale"] = scales
        out[base + ".input_scale"] = torch.tensor(0.5)  # activation quantization entries: ignored (W4A16)
        want[name] = deq.to(torch.bfloat16)
        assert torch.equal(want[name].double(), deq)
    if mutate:
        mutate(out)
    dst.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in out.items()}, str(dst / "model.safetensors"))
    cfg = json.loads((src / "config.json").read_text())
    cfg["quantization_config"] = {"quant_method": "quark", "weight": {"dtype": "fp4", "group_size": 32}}
    (dst / "config.json").write_text(json.dumps(cfg))
    return want


def _expect_layers(model, want):
    for i, L in enumerate(model.layers):
        p = f"model.layers.{i}."
        qkv = torch.cat([want[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        gu = torch.cat([want[p + "mlp.gate_proj.weight"], want[p + "mlp.up_proj.weight"]])
        for lin, w in ((L.qkv, qkv), (L.o, want[p + "self_attn.o_proj.weight"]), (L.gate_up, gu),
                       (L.down, want[p + "mlp.down_proj.weight"])):
            assert lin.kind == "mxfp4"
            assert torch.equal(lin.dense_weight(), w), (i, lin.layout)
        assert L.qkv.bias is not None and L.qkv.layout == "qkv" and L.gate_up.layout == "silu"
    assert model.lm_head.kind == "dense"


def test_oracles_agree_with_each_other_and_the_quantizer(dense_ckpt):
    _, tensors = dense_ckpt
    t = tensors["model.layers.0.self_attn.o_proj.weight"][:16]
    codes, scales, deq = _oracle_fast(t)
    slow, es = _oracle(t)
    assert torch.equal(slow, deq) and torch.equal(es, scales.long())
    c2, s2 = packing.mxfp4_quantize(t)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


def test_loader_reads_the_checkpoint_form(dense_ckpt, tmp_path):
    want = _write_mxfp4(dense_ckpt, tmp_path / "mx")
    model = DecoderModel(resolve_arch(str(tmp_path / "mx")), "cpu", weights_path=str(tmp_path / "mx"))
    _expect_layers(model, want)


def test_loader_takes_a_zero_block_with_scale_byte_0(dense_ckpt, tmp_path):
    k = "model.layers.1.mlp.down_proj"

    def mutate(out):
        out[k + ".weight"][7, 16:32] = 0x80  # block 1 of row 7 (k 32..63): codes +0 (low nibble) and -0 (high)
        out[k + ".weight_scale"][7, 1] = 0

    want = _write_mxfp4(dense_ckpt, tmp_path / "z", mutate)
    want[k + ".weight"][7, 32:64] = 0
    model = DecoderModel(resolve_arch(str(tmp_path / "z")), "cpu", weights_path=str(tmp_path / "z"))
    _expect_layers(model, want)


def _set_scale(name, n, kb, byte):
    def mutate(out):
        out[name][n, kb] = byte
    return mutate


def _drop(name):
    def mutate(out):
        del out[name]
    return mutate


def _reshape_scale(out):
    k = "model.layers.0.self_attn.o_proj.weight_scale"
    out[k] = out[k][:, :-1].contiguous()


def _odd_k(out):
    k = "model.layers.0.mlp.down_proj"
    out[k + ".weight"] = out[k + ".weight"][:, :-16].contiguous()  # K - 32: not a multiple of 128
    out[k + ".weight_scale"] = out[k + ".weight_scale"][:, :-1].contiguous()


@pytest.mark.parametrize("mutate,match", [
    (_set_scale("model.layers.1.mlp.up_proj.weight_scale", 3, 1, 255), r"layers\.1\.mlp\.up_proj\.weight_scale.*255"),
    (_set_scale("model.layers.0.self_attn.k_proj.weight_scale", 0, 0, 254), r"layers\.0\.self_attn\.k_proj\.weight_scale.*254"),
    (_set_scale("model.layers.0.self_attn.k_proj.weight_scale", 9, 2, 1), r"layers\.0\.self_attn\.k_proj\.weight_scale.*byte 1 "),
    (_drop("model.layers.0.self_attn.o_proj.weight_scale"), r"without model\.layers\.0\.self_attn\.o_proj\.weight_scale"),
    (_reshape_scale, r"layers\.0\.self_attn\.o_proj\.weight_scale: shape"),
    (_odd_k, r"layers\.0\.mlp\.down_proj\.weight: K = \d+ is not a multiple of 128"),
], ids=["nan_scale", "scale_254", "scale_1", "no_scale", "scale_shape", "k_not_128"])
def test_loader_rejects(dense_ckpt, tmp_path, mutate, match):
    _write_mxfp4(dense_ckpt, tmp_path / "bad", mutate)
    with pytest.raises(ValueError, match=match):
        DecoderModel(resolve_arch(str(tmp_path / "bad")), "cpu", weights_path=str(tmp_path / "bad"))


def test_loader_quantizes_a_bf16_checkpoint_at_load(dense_ckpt):
    src, tensors = dense_ckpt
    model = DecoderModel(resolve_arch(str(src)), "cpu", weights_path=str(src), quantization="mxfp4")
    for i, L in enumerate(model.layers):
        p = f"model.layers.{i}."
        assert all(lin.kind == "mxfp4" for lin in (L.qkv, L.o, L.gate_up, L.down))
        assert torch.equal(L.o.dense_weight().double(), _oracle_fast(tensors[p + "self_attn.o_proj.weight"])[2])
        assert torch.equal(L.down.dense_weight().double(), _oracle_fast(tensors[p + "mlp.down_proj.weight"])[2])
        qkv = torch.cat([tensors[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        assert torch.equal(L.qkv.dense_weight().double(), _oracle_fast(qkv)[2])
    assert model.lm_head.kind == "dense"
    dense = DecoderModel(resolve_arch(str(src)), "cpu", weights_path=str(src))
    assert all(L.qkv.kind == "dense" for L in dense.layers)


def test_save_checkpoint_writes_the_dequantised_bf16(dense_ckpt, tmp_path):
    want = _write_mxfp4(dense_ckpt, tmp_path / "mx")
    model = DecoderModel(resolve_arch(str(tmp_path / "mx")), "cpu", weights_path=str(tmp_path / "mx"))
    save_checkpoint(model, str(tmp_path / "deq"))
    back = load_file(str(tmp_path / "deq" / "model.safetensors"))
    for k, w in want.items():
        assert back[k].dtype == torch.bfloat16 and torch.equal(back[k], w), k


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


CPU_CFG = dict(model="tiny", device="cpu", max_model_len=256, max_num_seqs=8, max_num_batched_tokens=64,
               num_kv_blocks=64, warmup=False, seed=0)


def test_cpu_engine_mxfp4_equals_the_bf16_engine_on_dequantised_weights(tmp_path):
    """random_init under quantization='mxfp4': the dense branch's draws in MX blocks; greedy generation is
    token-equal to a bf16 engine loaded from the dequantised weights, and those are the quantizer's."""
    eng = LLMEngine(EngineConfig(quantization="mxfp4", **CPU_CFG))
    dense = LLMEngine(EngineConfig(**CPU_CFG))
    for Lq, Ld in zip(eng.model.layers, dense.model.layers):
        for a in ("qkv", "o", "gate_up", "down"):
            lq, ld = getattr(Lq, a), getattr(Ld, a)
            assert lq.kind == "mxfp4" and ld.kind == "dense" and lq.layout == ld.layout
            assert torch.equal(lq.dense_weight().double(), _oracle_fast(ld.dense_weight())[2])
    assert eng.model.lm_head.kind == "dense" and torch.equal(eng.model.embed, dense.model.embed)
    save_checkpoint(eng.model, str(tmp_path / "deq"))
    twin = LLMEngine(EngineConfig(**dict(CPU_CFG, model=str(tmp_path / "deq"))))
    assert all(L.down.kind == "dense" for L in twin.model.layers)
    toks = _greedy(eng, T.PROMPTS)
    assert toks == _greedy(twin, T.PROMPTS)
    assert toks != _greedy(dense, T.PROMPTS)  # 4-bit weights are another model than the bf16 draws


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
        assert all(lin.kind == "mxfp4" for L in eng.model.layers for lin in (L.qkv, L.o, L.gate_up, L.down))
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
def test_tp2_mxfp4_matches_tp1(dense_ckpt, tmp_path):
    """An MXFP4 checkpoint sharded over two gloo ranks (rows of qkv / gate_up, 128-multiple k-ranges of o /
    down with their scale bytes) generates the TP = 1 engine's tokens, every rank's matrices are the slices of
    the TP = 1 ones, and those are the oracle's."""
    from vgate.parallel.comm import TPGroup
    path = tmp_path / "ckpt"
    want = _write_mxfp4(dense_ckpt, path)
    e1 = LLMEngine(T._cfg(str(path), 1, dtype="float32"))
    _expect_layers(e1.model, want)
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
            assert all(lin.kind == "mxfp4" for lin in (Ls.qkv, Ls.o, Ls.gate_up, Ls.down))
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


# ------------------------------------------------------------------ the chat API
async def test_mxfp4_engine_serves_chat_completions():
    """An engine under quantization: mxfp4 behind /v1/chat/completions, both lanes: 200, six tokens, the same
    bytes on the fast lane and the FastAPI route."""
    be = NativeBackend.__new__(NativeBackend)
    be.watchdog_seconds = 60.0
    be.engine = LLMEngine(EngineConfig(quantization="mxfp4", **CPU_CFG))
    assert all(L.qkv.kind == "mxfp4" for L in be.engine.model.layers)
    be.engine.start()
    try:
        body = {"model": "m", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 6, "temperature": 0.0}
        out = []
        for fast in (True, False):
            c = VGateConfig(model={"quantization": "mxfp4"}, cache={"enabled": False})
            assert c.model.quantization == "mxfp4"
            eng = VGateEngine(model_config=c.model, worker_config=c.worker, backend=be, dry_run=True)
            app = create_app(c, engine=eng, fast_lane=fast)
            async with app.router.lifespan_context(app):
                async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                    r = await cl.post("/v1/chat/completions", json=body)
            assert r.status_code == 200, r.text
            j = r.json()
            assert j["usage"]["completion_tokens"] == 6 and j["choices"][0]["finish_reason"] == "length"
            out.append(j["choices"][0]["message"]["content"])
        assert out[0] == out[1] and isinstance(out[0], str)
    finally:
        be.engine.tp.size = 1
        be.engine.stop()
