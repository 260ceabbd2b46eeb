"""FP8 (e4m3 W8A16) on the GPU: the decode kernel (csrc/kernels/gemm_fp8.hip fp8_gemm_kernel) and the
fp8 -> bf16 scratch copy (fp8_dequant_packed_kernel), every output element.

The problems (tests/fp8_cases.py) are integers with power-of-two scales, so the expectation is one bit
pattern wherever the kernel applies the scale, splits K or rounds; buffers are the guarded, strided views
of tests/test_gemm_exact_gpu.py, whose helpers are imported. ``Linear.dense_weight()`` (checked on the CPU by
tests/test_fp8_cpu.py) is the reference of the Gaussian and engine tests."""
from __future__ import annotations

import functools
import math

import pytest
import torch

import fp8_cases as F
import gemm_exact as X
import test_engine_gpu as E
import test_gemm_exact_gpu as G
from vgate import ops
from vgate.ops import reference as ref
from vgate.runtime.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
F32_MODES = ("f32",)


def make_lin(p: F.Fp8Problem) -> ops.Linear:
    bias = p.bias.to(DEV) if p.bias is not None else None
    return ops.Linear(None, bias, fp8=dict(codes=p.fp8["codes"], scales=p.fp8["scales"].to(DEV), layout=p.kind))


@functools.lru_cache(maxsize=None)
def lin_for(s):
    p = F.build(s)
    return p, make_lin(p)


@pytest.fixture(autouse=True, scope="module")
def _native():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ops.native()
    yield
    lin_for.cache_clear()


def launch(p, lin, mode: str, knobs: dict, twice: bool = False) -> dict:
    """One C.gemm call of the fp8 decode kernel on guarded, strided buffers (the fp8 counterpart of
    test_gemm_exact_gpu.launch): timeline names, guard bytes, a bit-identical repeat, the fault word."""
    C = ops.native()
    M, N, K = p.M, p.N, p.K
    epi = 2 if p.kind == "silu" else 3 if p.kind == "qkv" else 1 if mode in F32_MODES else 0
    ncols = N // 2 if p.kind == "silu" else p.qkv["hq"] * 128 if p.kind == "qkv" else N
    kw = dict(ws=ops.workspace(DEV), fault=ops.fault_word(DEV), sk_ws=ops.sk_workspace(DEV), fp8_scales=lin.fscales,
              **knobs)
    xg = G.Guarded(M, K, init=p.x)
    og = G.Guarded(M, ncols, torch.float32 if mode in F32_MODES else BF16, init=p.res if mode == "inplace" else None)
    bufs = {"x": xg, "out": og}
    if mode in ("bias", "inplace", "f32") or p.kind == "qkv":
        kw["bias"] = lin.bias
    if mode == "res":
        bufs["res"] = G.Guarded(M, N, init=p.res, pad=40)
        kw["res"] = bufs["res"].view
    elif mode == "inplace":
        kw["res"] = og.view
    kc = vc = None
    if p.kind == "qkv":
        m = p.qkv
        kc = torch.full((m["blocks"], m["hkv"], m["bs"], 128), X.SENT, dtype=BF16, device=DEV)
        vc = kc.clone()
        kw.update(positions=m["positions"].to(DEV), slots=m["slots"].to(DEV), cos_sin=m["cos_sin"].to(DEV),
                  k_cache=kc, v_cache=vc, hq=m["hq"], hkv=m["hkv"])

    def go():
        C.gemm(xg.view, lin.wp, N, K, og.view, epi, **kw)

    fault0 = int(ops.fault_word(DEV)[0])
    ents = X.launches(go)
    r = {"names": [e[0] for e in ents], "blocks": [e[2] for e in ents]}
    what = f"fp8 {mode} {knobs} {r['names']}"
    for name, b in bufs.items():
        b.assert_guards(f"{what}: {name}")
    if twice:
        first = {k: b.big.clone() for k, b in bufs.items()}
        caches = (kc.clone(), vc.clone()) if kc is not None else None
        for b in bufs.values():
            b.reset()
        if caches:
            kc.fill_(X.SENT)
            vc.fill_(X.SENT)
        go()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert torch.equal(G.Guarded._bits(b.big), G.Guarded._bits(first[k])), f"{what}: second run differs in {k}"
        if caches:
            assert torch.equal(kc, caches[0]) and torch.equal(vc, caches[1]), f"{what}: second run differs in the cache"
    assert int(ops.fault_word(DEV)[0]) == fault0, f"{what}: fault word {int(ops.fault_word(DEV)[0])}"
    r["out"] = og.view.detach().cpu().double()
    if kc is not None:
        r["k_cache"], r["v_cache"] = kc, vc
    return r


# ------------------------------------------------------------------ every code
def _code_values():
    c = torch.arange(256, dtype=torch.uint8)
    c[(c & 0x7F) == 0x7F] = 0  # the two NaN codes
    return c.view(FP8)  # [256], index = code


def test_every_code_through_the_decode_kernel():
    """M = 16, N = 16, K = 512, one-hot x rows, W[n][k_m] = code 16 m + n, scale 1: out[m][n] is the value of
    that code — all 254 finite codes, subnormals down to 2^-9 and +-448, bit for bit (the sum 0 + (-0) of
    code 0x80 is +0: that one is compared by value)."""
    codes, x, _ = F.every_code_table()
    lin = ops.Linear(None, fp8=dict(codes=codes, scales=torch.ones(1, 16, device=DEV)))
    vals = _code_values().reshape(16, 16)  # [m][n]
    assert bool(torch.isfinite(vals.float()).all()) and float(vals.float().abs().max()) == 448.0
    assert float(vals.float().abs()[vals.float() != 0].min()) == 2.0 ** -9
    for f32 in (False, True):
        names = []
        y = None

        def go():
            nonlocal y
            y = ops.linear(x.to(DEV), lin, out_f32=f32)

        names = [e[0] for e in X.launches(go)]
        assert names == ["fp8_gemm"], names
        want = vals.float() if f32 else vals.to(BF16)
        got = y.cpu()
        bits = torch.int32 if f32 else torch.int16
        neg0 = torch.zeros(16, 16, dtype=torch.bool)
        neg0[8, 0] = True  # code 0x80
        assert torch.equal(got.view(bits)[~neg0], want.view(bits)[~neg0])
        assert float(got[8, 0]) == 0.0


def test_every_code_through_the_dequant():
    """The same table through fp8_dequant: bf16 of every code, -0 included, bit for bit; with a scale of
    2^-3 per channel the values scale exactly."""
    codes, _, km = F.every_code_table()
    C = ops.native()
    for s in (1.0, 0.125):
        lin = ops.Linear(None, fp8=dict(codes=codes, scales=torch.full((1, 16), s, device=DEV)))
        out = torch.full((16 * 512 + 256,), X.SENT, dtype=BF16, device=DEV)
        C.fp8_dequant(lin.wp, lin.fscales, 16, 512, out, None)
        torch.cuda.synchronize()
        w = ops.unpack_weight(out[: 16 * 512], 16, 512).cpu()
        want = (codes.view(FP8).float() * s).to(BF16)
        assert torch.equal(w.view(torch.int16), want.view(torch.int16))
        assert torch.equal(w[:, km].t().contiguous().view(torch.int16),
                           (_code_values().float() * s).to(BF16).reshape(16, 16).view(torch.int16))
        assert bool((out[16 * 512:] == X.SENT).all())


# ------------------------------------------------------------------ exact decode
DEC_PARAMS = [pytest.param(c, mode, form, id=f"{c[0]}-{mode}-{form}")
              for c in F.DEC_CASES for mode in F.DEC_MODES for form in F.SCALE_FORMS]


@pytest.mark.parametrize("c,mode,form", DEC_PARAMS)
@pytest.mark.parametrize("M", F.DEC_M)
def test_fp8_decode_exact(M, c, mode, form):
    """fp8_gemm at M <= 16: the launcher's own plan and forced K slices (2: granules, 3 / 8: slabs + ticket)
    with 2 / 4 waves, one / two / four tiles per block, per-channel and 128-block scales, every epilogue;
    every element, guard bytes, the launch's name and grid, a bit-identical repeat, the fault word."""
    _, N, K, knobs = c
    s = F.spec_for(mode, M, N, K, form)
    p, lin = lin_for(s)
    assert lin.fscales.shape[0] == (1 if form == "channel" else K // 128)
    r = launch(p, lin, mode, knobs, twice=True)
    what = f"{s} {mode} {knobs}"
    assert r["names"] == ["fp8_gemm"], f"{what}: launched {r['names']}"
    if knobs:
        KQ = K // 128
        nsl = min(knobs["splitk"], 8)
        while nsl > 1 and KQ // nsl < 1:
            nsl >>= 1
        ntb = knobs.get("ntb", 1)
        if mode == "qkv" or (p.N // 16) % ntb:
            ntb = 1
        assert r["blocks"] == [(p.N // 16) // ntb * nsl], (what, r["blocks"])
    G.assert_exact(r["out"], G.expected(p, mode), what)
    if mode == "qkv":
        assert torch.equal(r["k_cache"].cpu().double(), p.exp["k_cache"]), what + " k_cache"
        assert torch.equal(r["v_cache"].cpu().double(), p.exp["v_cache"]), what + " v_cache"


@pytest.mark.parametrize("M,mode,form", F.WIDE_CASES)
def test_fp8_wide_n_runs_tile_pairs(M, mode, form):
    """N of 1026 tiles on the launcher's own plan: two tiles per block (gemm_fp8.hip fp8_ntb_rule), exact."""
    p, lin = lin_for(F.spec_for(mode, M, F.WIDE_N, 512, form))
    r = launch(p, lin, mode, {}, twice=True)
    assert r["names"] == ["fp8_gemm"] and r["blocks"][0] % (p.N // 32) == 0, (r["names"], r["blocks"], p.N // 32)
    assert r["blocks"][0] // (p.N // 32) <= 8
    G.assert_exact(r["out"], G.expected(p, mode), f"wide {M} {mode} {form}")


@pytest.mark.parametrize("form", F.SCALE_FORMS)
@pytest.mark.parametrize("M,N,K,knobs", [(8, 256, 512, dict(waves=4, splitk=2)), (5, F.ODD_N, 1536, {})])
def test_one_wrong_code_is_seen(M, N, K, knobs, form):
    """One code of the last output column replaced: the exact comparison fails in exactly that column."""
    p, _ = lin_for(F.spec_for("bias", M, N, K, form))
    n, k = p.N - 1, X.active_k(p, p.K // 2)
    pp = F.perturb(p, n, k)
    r = launch(pp, make_lin(pp), "bias", knobs)
    assert r["names"] == ["fp8_gemm"]
    want = G.expected(p, "bias")
    bad = r["out"] != want
    hit = torch.zeros_like(bad)
    hit[:, n] = p.x[:, k].double() != 0
    assert bool(hit.any()) and torch.equal(bad, hit), f"wrong elements {bad.nonzero()[:8].tolist()}"


# ------------------------------------------------------------------ dequant + the bf16 kernels (M > 16)
@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("form", F.SCALE_FORMS)
@pytest.mark.parametrize("N,K", F.DEQ_SHAPES)
def test_fp8_dequant_exact(N, K, form, gamma):
    """bf16(code * s [* gamma]) element for element in the packed order ops.unpack_weight undoes; nothing
    past N * K elements is written."""
    p, lin = lin_for(F.spec_for("bias", 17, N, K, form))
    out = torch.full((N * K + 256,), X.SENT, dtype=BF16, device=DEV)
    g = None
    want = p.w.double()
    if gamma:
        g = 2.0 ** torch.randint(-1, 2, (K,), generator=X._gen(K)).double()
        want = want * g[None]
        g = g.to(BF16).to(DEV)
    ops.native().fp8_dequant(lin.wp, lin.fscales, N, K, out, g)
    torch.cuda.synchronize()
    G.assert_exact(ops.unpack_weight(out[: N * K], N, K), want, "fp8_dequant")
    assert bool((out[N * K:] == X.SENT).all())


@pytest.mark.parametrize("form", F.SCALE_FORMS)
@pytest.mark.parametrize("N,K", F.DEQ_SHAPES)
@pytest.mark.parametrize("M", F.DEQ_M)
def test_fp8_route_above_16_rows(M, N, K, form):
    """ops.linear on an fp8 Linear at M > 16: the dequant, then exactly the bf16 launches the route names
    for a dense Linear of that shape; every element."""
    p, lin = lin_for(F.spec_for("bias", M, N, K, form))
    dense = ops.Linear(p.w.to(DEV), bias=lin.bias)
    route = ops._gemm_route(lin, M, waves=0, splitk=0, path=0, row_idx=None, ar=None, norm_out=None)
    assert route == ("dequant", {})
    x = p.x.to(DEV)
    out = {}

    def run(key, l):
        def go():
            out[key] = ops.linear(x, l)
        return [e[0] for e in X.launches(go)]

    names_fp8, names_dense = run("fp8", lin), run("dense", dense)
    assert names_fp8 == names_dense and len(names_fp8) >= 1 and "fp8_gemm" not in names_fp8, (names_fp8, names_dense)
    G.assert_exact(out["fp8"], p.exp["biased"], f"fp8 route M={M} {names_fp8}")


# ------------------------------------------------------------------ Gaussian data, quantize_fp8, fused RMSNorm
def _gauss(N, K, M, seed, layout="plain", bias=False):
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV).bfloat16()
    nw = (torch.rand(K, device=DEV) + 0.5).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    b = (torch.randn(N, device=DEV) * 0.1).bfloat16() if bias else None
    lin = ops.Linear.quantize_fp8(w, bias=b, layout=layout)
    assert lin.kind == "fp8" and lin.wp.dtype == torch.uint8 and lin.fscales.shape == (1, N)
    assert lin.nbytes() == N * K + 4 * N
    xn, _ = ref.rmsnorm_ref(x, nw, 1e-6)
    return x, nw, lin, lin.dense_weight(), xn


@pytest.mark.parametrize("M", [7, 16])
def test_gaussian_bf16_and_f32(M):
    x, nw, lin, wd, xn = _gauss(1024, 1536, M, 21)
    r = torch.randn(M, 1024, device=DEV).bfloat16()
    y = ops.linear(x, lin, residual=r, norm=(nw, 1e-6))
    assert X.rel_err(y, ref.linear_ref(xn, wd, None, r)) < 1e-2
    y32 = ops.linear(x, lin, out_f32=True, norm=(nw, 1e-6))
    assert y32.dtype == torch.float32
    assert X.rel_err(y32, ref.linear_ref(xn, wd, out_f32=True)) < 5e-3
    y2 = ops.linear(x, lin, residual=r, norm=(nw, 1e-6), splitk=3, waves=4)
    assert X.rel_err(y2, ref.linear_ref(xn, wd, None, r)) < 1e-2


def test_gaussian_silu():
    x, nw, lin, wd, xn = _gauss(1024, 1536, 9, 22, layout="silu")
    y = ops.linear(x, lin, norm=(nw, 1e-6))
    assert X.rel_err(y, ref.silu_mul_linear_ref(xn, wd[:512], wd[512:])) < 1e-2


def test_gaussian_qkv():
    hq, hkv, D, BS, T = 4, 2, 128, 16, 13
    x, nw, lin, wd, xn = _gauss((hq + 2 * hkv) * D, 1536, T, 23, layout="qkv", bias=True)
    pos = torch.randint(0, 1000, (T,), dtype=torch.int32, device=DEV)
    slots = torch.randperm(32 * BS, device=DEV)[:T].int()
    slots[4] = -1
    cs = ref.rope_cos_sin(1024, D, 1e6, device=DEV)
    kc = torch.zeros(32, hkv, BS, D, device=DEV).bfloat16()
    vc = torch.zeros_like(kc)
    q = ops.linear(x, lin, norm=(nw, 1e-6), qkv=dict(positions=pos, slots=slots, cos_sin=cs, k_cache=kc, v_cache=vc,
                                                     hq=hq, hkv=hkv))
    qkv = ref.linear_ref(xn, wd, lin.bias)
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    ref.rope_kv_ref(qkv, pos, slots, cs, kc2, vc2, hq, hkv, D)
    assert X.rel_err(q, qkv[:, : hq * D]) < 1e-2
    assert X.rel_err(kc, kc2) < 1e-2 and X.rel_err(vc, vc2) < 1e-2


def test_gaussian_prefill_rows_fold_gamma_in_the_scratch():
    """M > 16 with norm=(gamma, eps): gamma is folded into the dequantised scratch and the bf16 kernels
    apply the row scale alone."""
    for M in (40, 200):
        x, nw, lin, wd, xn = _gauss(1024, 1536, M, 24)
        y = ops.linear(x, lin, norm=(nw, 1e-6))
        assert X.rel_err(y, ref.linear_ref(xn, wd)) < 1e-2


# ------------------------------------------------------------------ declines
def test_declines():
    p, lin = lin_for(F.spec_for("bias", 5, 256, 512, "channel"))
    C = ops.native()
    x = torch.zeros(13, 512, dtype=BF16, device=DEV)
    out = torch.zeros(5, 256, dtype=BF16, device=DEV)
    out32 = torch.zeros(5, 256, dtype=torch.float32, device=DEV)
    idx = torch.arange(5, dtype=torch.int32, device=DEV)
    kw = dict(ws=ops.workspace(DEV), fp8_scales=lin.fscales)
    with pytest.raises(RuntimeError, match="row_idx"):
        C.gemm(x, lin.wp, 256, 512, out32, 1, row_idx=idx, **kw)
    with pytest.raises(ValueError, match="row_idx"):
        ops.linear(x, lin, out_f32=True, row_idx=idx)
    with pytest.raises(RuntimeError, match="all-reduce"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, ar_bases=[0], ar_rank=0, ar_fused_off=1 << 20, **kw)

    class FakeAr:
        bases, rank, fused_off = [0], 0, 1 << 20

    with pytest.raises(ValueError, match="all-reduce"):
        ops.linear(x[:5], lin, ar=FakeAr())
    with pytest.raises(RuntimeError, match="M <= 16"):
        C.gemm(torch.zeros(17, 512, dtype=BF16, device=DEV), lin.wp, 256, 512, torch.zeros(17, 256, dtype=BF16, device=DEV),
               0, **kw)
    with pytest.raises(RuntimeError, match="scales"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, ws=ops.workspace(DEV), fp8_scales=torch.ones(2, 256, device=DEV))
    with pytest.raises(RuntimeError, match="numel"):
        C.gemm(x[:5], lin.wp[:-1], 256, 512, out, 0, **kw)
    with pytest.raises(RuntimeError, match="hand-off"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, ssp_out=torch.zeros(5 * 16, device=DEV), **kw)
    with pytest.raises(ValueError, match="K % 128"):
        ops.Linear(None, fp8=dict(codes=torch.zeros(16, 192, dtype=torch.uint8), scales=torch.ones(1, 16, device=DEV)))
    assert int(ops.fault_word(DEV)[0]) == 0


# ------------------------------------------------------------------ engine
def test_fp8_engine_graph_eager_reference_and_mixed_step():
    """quantization='fp8' end to end: generation under hipGraphs equals eager, both are the (near-)argmax of
    the teacher-forced fp32 forward on the dequantised weights (the AWQ engine test's margin), the weights
    are half the bf16 model's layer bytes, and a prompt that arrives while others decode (a mixed prefill +
    decode step: every row on the dequantised scratch + the bf16 kernels) keeps all three within that margin."""
    eng = E._engine(quantization="fp8")
    assert all(lin.kind == "fp8" and lin.wp.dtype == torch.uint8
               for L in eng.model.layers for lin in (L.qkv, L.o, L.gate_up, L.down))
    assert eng.model.weight_bytes() < E._engine().model.weight_bytes()
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    reqs = [(k, v, sp) for k, v in list(E.PROMPTS.items())[:3]]
    g = E._run(eng, reqs)
    assert eng.runner.graph_hits > 0
    e = E._run(E._engine(quantization="fp8", enforce_eager=True), reqs)
    for k, ids in list(E.PROMPTS.items())[:3]:
        assert len(g[k].output_ids) == 12 and g[k].output_ids == e[k].output_ids, k
        logits = eng.model.reference_logits(ids + g[k].output_ids[:-1])[len(ids) - 1:]
        for t, tok in enumerate(g[k].output_ids):
            row = logits[t]
            assert row[tok] >= row.max() - 0.05 * row.std(), (k, t)
    # mixed step: q0 and q1 decode, then q5 (52 tokens) is prefilled beside their decode rows
    eng2 = E._engine(quantization="fp8")
    done = {}

    def cb(kind, seq, payload):
        done[seq.request_id] = seq

    for k in ("q0", "q1"):
        eng2.add_request(k, params=sp, callback=cb, prompt_ids=E.PROMPTS[k])
    eng2._drain_inbox()
    for _ in range(3):
        assert eng2.step() == 2
    eng2.add_request("q5", params=sp, callback=cb, prompt_ids=E.PROMPTS["q5"])
    eng2._drain_inbox()
    assert eng2.step() == 3  # the mixed step: two decode rows + the 52-token prompt
    eng2.run_until_idle()
    for k in ("q0", "q1", "q5"):
        ids, toks = E.PROMPTS[k], done[k].output_ids
        assert len(toks) == 12
        logits = eng2.model.reference_logits(ids + toks[:-1])[len(ids) - 1:]
        for t, tok in enumerate(toks):
            assert logits[t][tok] >= logits[t].max() - 0.05 * logits[t].std(), (k, t)
