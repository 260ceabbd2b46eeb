"""MXFP4 (e2m1 W4A16, e8m0 block-32 scales) on the GPU: the decode kernel (csrc/kernels/gemm_mxfp4.hip
mxfp4_gemm_kernel) and the mxfp4 -> bf16 scratch copy (mxfp4_dequant_packed_kernel), every output element.

The problems (tests/mxfp4_cases.py) are integers with power-of-two block scales that vary per (row, block),
so the expectation is one bit pattern however the kernel splits K or groups tiles; buffers are the guarded,
strided views of tests/test_gemm_exact_gpu.py, whose helpers are imported. ``Linear.dense_weight()`` (exact
in bf16, checked on the CPU by tests/test_mxfp4_cpu.py) is the reference of the Gaussian and engine tests."""
from __future__ import annotations

import functools
import math

import pytest
import torch

import gemm_exact as X
import mxfp4_cases as F
import test_engine_gpu as E
import test_gemm_exact_gpu as G
from vgate import ops
from vgate.models.weights import save_checkpoint
from vgate.ops import reference as ref
from vgate.runtime.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
F32_MODES = ("f32",)
NAME = "mxfp4_gemm"


def make_lin(p: F.Mxfp4Problem) -> ops.Linear:
    bias = p.bias.to(DEV) if p.bias is not None else None
    return ops.Linear(None, bias, mxfp4=dict(codes=p.mxfp4["codes"], scales=p.mxfp4["scales"].to(DEV), layout=p.kind))


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
    """One C.gemm call of the mxfp4 decode kernel on guarded, strided buffers (the counterpart of
    test_gemm_exact_gpu.launch): timeline names, guard bytes, a bit-identical repeat, the fault word."""
    C = ops.native()
    M, N, K = p.M, p.N, p.K
    epi = 2 if p.kind == "silu" else 3 if p.kind == "qkv" else 1 if mode in F32_MODES else 0
    ncols = N // 2 if p.kind == "silu" else p.qkv["hq"] * 128 if p.kind == "qkv" else N
    kw = dict(ws=ops.workspace(DEV), fault=ops.fault_word(DEV), sk_ws=ops.sk_workspace(DEV),
              mxfp4_scales=lin.mscales, **knobs)
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
    what = f"mxfp4 {mode} {knobs} {r['names']}"
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
def test_every_code_through_the_decode_kernel():
    """M = 16, N = 16, K = 512, one-hot x rows in 16 distinct blocks, row n = code n, block m at scale byte
    EVERY_CODE_SCALES[m] (2 .. 252): out[m][n] = value(n) x 2^(e_m - 127) in the f32 epilogue, all 16 codes at
    all 16 scales, compared numerically (the sum 0 + (-0) of code 8 is +0). This is what establishes how the
    scaled conversion instruction treats its scale operand on the hardware."""
    codes, scales, x, _ = F.every_code_table()
    lin = ops.Linear(None, mxfp4=dict(codes=codes, scales=scales.to(DEV)))
    want = F.every_code_values()
    assert float(want.abs().max()) == 6.0 * 2.0 ** 125 and float(want.abs()[want != 0].min()) == 2.0 ** -126
    y = None

    def go():
        nonlocal y
        y = ops.linear(x.to(DEV), lin, out_f32=True)

    names = [e[0] for e in X.launches(go)]
    assert names == [NAME], names
    assert y.dtype == torch.float32
    got = y.cpu().double()
    bad = (got != want).nonzero().tolist()
    assert not bad, [(m, n, float(got[m, n]), float(want[m, n])) for m, n in bad[:8]]


@pytest.mark.parametrize("gamma", [False, True])
def test_every_code_through_the_dequant(gamma):
    """The same table through mxfp4_dequant: bf16 of every code at every scale, -0 included, bit for bit.
    With a gamma whose products need more than bf16's 8 significant bits (1 + 2^-7 under the scales <= 2,
    0.7578125 under the larger ones, so every product stays normal and finite): bf16 of the fp32 product,
    one rounding, against torch's rounding of the same fp32 product."""
    codes, scales, _, km = F.every_code_table()
    C = ops.native()
    lin = ops.Linear(None, mxfp4=dict(codes=codes, scales=scales.to(DEV)))
    out = torch.full((16 * 512 + 256,), X.SENT, dtype=BF16, device=DEV)
    g = torch.where(torch.arange(512) < 256, 1.0078125, 0.7578125).to(BF16) if gamma else None
    C.mxfp4_dequant(lin.wp, lin.mscales, 16, 512, out, g.to(DEV) if gamma else None)
    torch.cuda.synchronize()
    w = ops.unpack_weight(out[: 16 * 512], 16, 512).cpu()
    want = torch.zeros(16, 512, dtype=torch.float64)
    want[:, km] = F.every_code_values().t()  # [n][m]; row 8 is -0 at every k_m
    want = want.float()
    if gamma:
        assert torch.equal(g.double(), torch.where(torch.arange(512) < 256, 1.0078125, 0.7578125).double())
        want = want * g.float()[None]
        assert bool(torch.isfinite(want).all()) and float(want.abs()[want != 0].min()) >= 2.0 ** -126
        assert not torch.equal(want.to(BF16).float(), want)  # the product does round
    want = want.to(BF16)
    assert torch.equal(w.view(torch.int16), want.view(torch.int16))
    assert int(w.view(torch.int16)[8, km[0]]) == -32768  # -0 kept
    assert bool((out[16 * 512:] == X.SENT).all())


# ------------------------------------------------------------------ exact decode
DEC_PARAMS = [pytest.param(c, mode, id=f"{c[0]}-{mode}") for c in F.DEC_CASES for mode in F.DEC_MODES]


@pytest.mark.parametrize("c,mode", DEC_PARAMS)
@pytest.mark.parametrize("M", F.DEC_M)
def test_mxfp4_decode_exact(M, c, mode):
    """mxfp4_gemm at M <= 16: the launcher's own plan and forced K slices (2: granules, 3 / 8: slabs + ticket)
    with 2 / 4 waves, one / two / four tiles per block, every epilogue; every element, guard bytes, the
    launch's name and grid, a bit-identical repeat, the fault word."""
    _, N, K, knobs = c
    s = F.spec_for(mode, M, N, K)
    p, lin = lin_for(s)
    r = launch(p, lin, mode, knobs, twice=True)
    what = f"{s} {mode} {knobs}"
    assert r["names"] == [NAME], f"{what}: launched {r['names']}"
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


@pytest.mark.parametrize("M,mode,N,ntb", F.WIDE_CASES)
def test_mxfp4_wide_n_follows_the_default_tile_rule(M, mode, N, ntb):
    """N just above a tile count at which the launcher's own rule (gemm_mxfp4.hip mxfp4_ntb_rule) changes, one
    K slice forced and the tile count left to the rule: the block count is tiles / ntb; exact."""
    p, lin = lin_for(F.spec_for(mode, M, N, 512))
    r = launch(p, lin, mode, dict(waves=4, splitk=1), twice=True)
    assert r["names"] == [NAME] and r["blocks"] == [p.N // 16 // ntb], (r["names"], r["blocks"], p.N // 16, ntb)
    G.assert_exact(r["out"], G.expected(p, mode), f"wide {M} {mode} {N}")


@pytest.mark.parametrize("M,N,K,knobs", [(8, 256, 512, dict(waves=4, splitk=2)), (5, F.ODD_N, 1536, {})])
def test_one_wrong_code_is_seen(M, N, K, knobs):
    """One code of the last output column replaced: the exact comparison fails in exactly that column."""
    p, _ = lin_for(F.spec_for("bias", M, N, K))
    n, k = p.N - 1, F.active_code(p, p.N - 1, p.K // 2)
    pp = F.perturb(p, n, k)
    r = launch(pp, make_lin(pp), "bias", knobs)
    assert r["names"] == [NAME]
    bad = r["out"] != G.expected(p, "bias")
    hit = torch.zeros_like(bad)
    hit[:, n] = p.x[:, k].double() != 0
    assert bool(hit.any()) and torch.equal(bad, hit), f"wrong elements {bad.nonzero()[:8].tolist()}"
    G.assert_exact(r["out"], G.expected(pp, "bias"), "perturbed code")


@pytest.mark.parametrize("M,N,K,knobs", [(8, 256, 512, dict(waves=4, splitk=2)), (5, F.ODD_N, 1536, {})])
def test_one_wrong_scale_is_seen(M, N, K, knobs):
    """One block's scale byte of one output column (the first from 17 on that x reaches) moved by one: exactly
    that column changes, in the rows whose x reaches the block; the new values are the perturbed problem's."""
    p, _ = lin_for(F.spec_for("bias", M, N, K))
    n, kb = F.active_block(p, 17)
    pp = F.perturb_scale(p, n, kb)
    r = launch(pp, make_lin(pp), "bias", knobs)
    assert r["names"] == [NAME]
    bad = r["out"] != G.expected(p, "bias")
    hit = pp.exp["biased"] != p.exp["biased"]
    assert bool(hit.any()) and not bool(hit[:, :n].any()) and not bool(hit[:, n + 1:].any())
    assert torch.equal(bad, hit), f"wrong elements {bad.nonzero()[:8].tolist()}"
    G.assert_exact(r["out"], G.expected(pp, "bias"), "perturbed scale")


# ------------------------------------------------------------------ dequant + the bf16 kernels (M > 16)
@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("N,K", F.DEQ_SHAPES)
def test_mxfp4_dequant_exact(N, K, gamma):
    """bf16(value * 2^(e-127) [* gamma]) element for element in the packed order ops.unpack_weight undoes;
    nothing past N * K elements is written."""
    p, lin = lin_for(F.spec_for("bias", 17, N, K))
    out = torch.full((N * K + 256,), X.SENT, dtype=BF16, device=DEV)
    g = None
    want = p.w.double()
    if gamma:
        g = 2.0 ** torch.randint(-1, 2, (K,), generator=X._gen(K)).double()
        want = want * g[None]
        g = g.to(BF16).to(DEV)
    ops.native().mxfp4_dequant(lin.wp, lin.mscales, N, K, out, g)
    torch.cuda.synchronize()
    G.assert_exact(ops.unpack_weight(out[: N * K], N, K), want, "mxfp4_dequant")
    assert bool((out[N * K:] == X.SENT).all())


@pytest.mark.parametrize("N,K", F.DEQ_SHAPES)
@pytest.mark.parametrize("M", F.DEQ_M)
def test_mxfp4_route_above_16_rows(M, N, K):
    """ops.linear on an mxfp4 Linear at M > 16: the dequant, then exactly the bf16 launches the route names
    for a dense Linear of that shape; every element."""
    p, lin = lin_for(F.spec_for("bias", M, N, K))
    dense = ops.Linear(p.w.to(DEV), bias=lin.bias)
    route = ops._gemm_route(lin, M, waves=0, splitk=0, path=0, row_idx=None, ar=None, norm_out=None)
    assert route == ("dequant", {})
    x = p.x.to(DEV)
    out = {}

    def run(key, l):
        def go():
            out[key] = ops.linear(x, l)
        return [e[0] for e in X.launches(go)]

    names_mx, names_dense = run("mx", lin), run("dense", dense)
    assert names_mx == names_dense and len(names_mx) >= 1 and NAME not in names_mx, (names_mx, names_dense)
    G.assert_exact(out["mx"], p.exp["biased"], f"mxfp4 route M={M} {names_mx}")


# ------------------------------------------------------------------ Gaussian data, quantize_mxfp4, fused RMSNorm
# (the reference and tolerances of tests/test_fp8_gpu.py's Gaussian tests: the arithmetic after the conversion
# is the same bf16 x bf16 MFMA with fp32 accumulation against the same kind of exact bf16 dense_weight())
def _gauss(N, K, M, seed, layout="plain", bias=False):
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV).bfloat16()
    nw = (torch.rand(K, device=DEV) + 0.5).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    b = (torch.randn(N, device=DEV) * 0.1).bfloat16() if bias else None
    lin = ops.Linear.quantize_mxfp4(w, bias=b, layout=layout)
    assert lin.kind == "mxfp4" and lin.wp.dtype == torch.uint8 and lin.mscales.dtype == torch.uint8
    assert lin.wp.numel() == N * K // 2 and lin.mscales.numel() == N * K // 32
    assert lin.nbytes() == N * K // 2 + N * K // 32
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
    p, lin = lin_for(F.spec_for("bias", 5, 256, 512))
    C = ops.native()
    x = torch.zeros(13, 512, dtype=BF16, device=DEV)
    out = torch.zeros(5, 256, dtype=BF16, device=DEV)
    out32 = torch.zeros(5, 256, dtype=torch.float32, device=DEV)
    idx = torch.arange(5, dtype=torch.int32, device=DEV)
    kw = dict(ws=ops.workspace(DEV), mxfp4_scales=lin.mscales)
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
    with pytest.raises(ValueError, match="hand-off"):
        ops.linear(x[:5], lin, norm_out=(None, None, None))
    with pytest.raises(RuntimeError, match="M <= 16"):
        C.gemm(torch.zeros(17, 512, dtype=BF16, device=DEV), lin.wp, 256, 512, torch.zeros(17, 256, dtype=BF16, device=DEV),
               0, **kw)
    with pytest.raises(RuntimeError, match="scales"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, ws=ops.workspace(DEV),
               mxfp4_scales=torch.zeros(2, 256, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="numel"):
        C.gemm(x[:5], lin.wp.reshape(-1)[:-16], 256, 512, out, 0, **kw)
    with pytest.raises(RuntimeError, match="hand-off"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, ssp_out=torch.zeros(5 * 16, device=DEV), **kw)
    with pytest.raises(RuntimeError, match="fused-attention"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, fa_out=torch.zeros(5, 256, dtype=BF16, device=DEV), **kw)
    with pytest.raises(RuntimeError, match="exclusive"):
        C.gemm(x[:5], lin.wp, 256, 512, out, 0, fp8_scales=torch.ones(1, 256, device=DEV), **kw)
    with pytest.raises(ValueError, match="K % 128"):
        ops.Linear(None, mxfp4=dict(codes=torch.zeros(16, 192, dtype=torch.uint8),
                                    scales=torch.full((16, 6), 127, dtype=torch.uint8, device=DEV)))
    assert int(ops.fault_word(DEV)[0]) == 0


# ------------------------------------------------------------------ engine
def test_mxfp4_engine_graph_eager_bf16_twin_and_mixed_step(tmp_path):
    """quantization='mxfp4' end to end: generation under hipGraphs, eager, and a bf16 engine loaded from the
    checkpoint save_checkpoint writes (the dequantised weights, exact in bf16) agree token for token, also
    across a mixed step (two decode rows beside a 52-token prompt: every row on the dequantised scratch + the
    bf16 kernels); the layers stream under a third of the bf16 model's bytes."""
    eng = E._engine(quantization="mxfp4")
    lins = [lin for L in eng.model.layers for lin in (L.qkv, L.o, L.gate_up, L.down)]
    assert all(lin.kind == "mxfp4" and lin.wp.dtype == torch.uint8 for lin in lins)
    assert eng.model.lm_head.kind == "dense"
    assert all(lin.nbytes() == lin.N * lin.K // 2 + lin.N * lin.K // 32 for lin in lins)
    save_checkpoint(eng.model, str(tmp_path / "deq"))
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    reqs = [(k, v, sp) for k, v in list(E.PROMPTS.items())[:3]]
    g = E._run(eng, reqs)
    assert eng.runner.graph_hits > 0
    e = E._run(E._engine(quantization="mxfp4", enforce_eager=True), reqs)
    twin = E._engine(model=str(tmp_path / "deq"))
    assert all(lin.kind == "dense" for L in twin.model.layers for lin in (L.qkv, L.o, L.gate_up, L.down))
    for La, Lb in zip(eng.model.layers, twin.model.layers):
        assert torch.equal(La.down.dense_weight(), Lb.down.dense_weight())
    b = E._run(twin, reqs)
    for k, _ in list(E.PROMPTS.items())[:3]:
        assert len(g[k].output_ids) == 12
        assert g[k].output_ids == e[k].output_ids == b[k].output_ids, k

    def mixed(en):
        done = {}

        def cb(kind, seq, payload):
            done[seq.request_id] = seq

        for k in ("q0", "q1"):
            en.add_request(k, params=sp, callback=cb, prompt_ids=E.PROMPTS[k])
        en._drain_inbox()
        for _ in range(3):
            assert en.step() == 2
        en.add_request("q5", params=sp, callback=cb, prompt_ids=E.PROMPTS["q5"])
        en._drain_inbox()
        assert en.step() == 3  # the mixed step: two decode rows + the 52-token prompt
        en.run_until_idle()
        return {k: done[k].output_ids for k in ("q0", "q1", "q5")}

    mg = mixed(E._engine(quantization="mxfp4"))
    me = mixed(E._engine(quantization="mxfp4", enforce_eager=True))
    mb = mixed(E._engine(model=str(tmp_path / "deq")))
    assert all(len(v) == 12 for v in mg.values())
    assert mg == me == mb
