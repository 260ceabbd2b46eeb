"""Every GEMM family on integer problems: the kernel that ran, every output element, every guard byte.

The older kernel tests compare norm-wise on Gaussian data, never ask which kernel a forcing knob
reached, and allocate every operand at its exact size. Here (helpers: tests/gemm_exact.py)

* the operands are small integers, so the expected output is one bit pattern for any summation
  order, K split or tile shape, computed on the CPU in float64;
* every case names the launches it means to hit (the ``tl_take`` names of the launch timeline) and a
  launcher that declines a shape / mode is written down as such, with the fallback's name;
* ``x``, ``out``, ``res`` and the hand-off outputs are views inside sentinel-filled allocations with
  a row stride wider than the row, and every byte outside the logical output must survive.

Findings fixed with this file: a forced ``ntb=2`` on an odd tile count left the last 16 columns
unwritten (gemm_decode.h dispatch_epi: now one tile per block); ``path=2, waves=8`` and ``path=1`` at
<= 16 rows dropped the RMSNorm hand-off outputs (gemm_mid.hip / gemm_prefill.hip: they now decline such
a launch and the decode kernels run it); ``row_idx`` under a bf16 epilogue was ignored by the decode
kernels, which computed rows 0..M-1 instead (bindings.cpp: rejected, the f32 LM-head form stays).
No family assumed contiguous rows: every one passes with padded row strides.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import pytest
import torch

import gemm_exact as X
from vgate import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16

# ------------------------------------------------------------------ problems (built on the CPU too)
SPECS: set = set()
_BUILDERS = {"dense": X.dense_problem, "awq": X.awq_problem, "silu": X.silu_problem,
             "awq_silu": X.awq_silu_problem, "qkv": X.qkv_problem}
QKV_HEADS = {512: (2, 1), 640: (3, 1)}  # N of the QKV epilogue -> (hq, hkv)


def spec_for(mode: str, M: int, N: int, K: int, awq: bool = False, group: int = 128):
    """The problem of one (epilogue mode, shape); registered for the CPU companion."""
    if mode == "silu":
        s = ("awq_silu" if awq else "silu", M, N // 2, K)
    elif mode == "qkv":
        s = ("qkv", M) + QKV_HEADS.get(N, (2, 1)) + (K, awq)
    elif awq:
        s = ("awq", M, N, K, group)
    else:
        s = ("dense", M, N, K)
    SPECS.add(s)
    return s


def build(s) -> X.Problem:
    return _BUILDERS[s[0]](*s[1:])


def make_lin(p: X.Problem) -> ops.Linear:
    bias = p.bias.to(DEV) if p.bias is not None else None
    if p.awq is not None:
        a = p.awq
        return ops.Linear(None, bias=bias, awq=dict(qint=a["qint"], scales=a["scales"].to(DEV), zeros=a["zeros"].to(DEV),
                                                    group=a["group"], layout=p.kind))
    return ops.Linear(p.w.to(DEV), bias=bias, layout=p.kind)


@functools.lru_cache(maxsize=None)
def lin_for(s):
    p = build(s)
    return p, make_lin(p)


@pytest.fixture(autouse=True, scope="module")
def _native():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ops.native()  # must load: no silent fallback
    yield
    lin_for.cache_clear()


# ------------------------------------------------------------------ guarded, strided buffers
class Guarded:
    """``view`` [rows, cols] inside a sentinel-filled allocation: GUARD rows before and after, and
    (strided) a row stride of cols rounded up to 8 plus ``pad`` elements."""

    def __init__(self, rows, cols, dtype=BF16, init=None, strided=True, pad=24):
        ld = (cols + 7) // 8 * 8 + (pad if strided else 0)
        self.big = torch.full((rows + 2 * X.GUARD, ld), X.SENT, dtype=dtype, device=DEV)
        self.view = self.big[X.GUARD:X.GUARD + rows, :cols]
        self.mask = torch.ones_like(self.big, dtype=torch.bool)
        self.mask[X.GUARD:X.GUARD + rows, :cols] = False
        if init is not None:
            self.view.copy_(init.to(DEV))
        self.before = self.big.clone()

    @staticmethod
    def _bits(t):
        return t.view(torch.int16 if t.dtype == BF16 else torch.int32)

    def reset(self):
        self.big.copy_(self.before)

    def assert_guards(self, what):
        a, b = self._bits(self.big)[self.mask], self._bits(self.before)[self.mask]
        if not torch.equal(a, b):
            idx = (self._bits(self.big) != self._bits(self.before)) & self.mask
            rc = idx.nonzero()
            raise AssertionError(f"{what}: {len(rc)} guard elements overwritten, first (row, col) "
                                 f"{rc[:6].tolist()} of {tuple(self.big.shape)} (view starts at row {X.GUARD})")


def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Every element equal by value (0 * negative is -0)."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    dims = [sorted(set(bad[:, d].tolist())) for d in range(bad.shape[1])]
    i = tuple(bad[0].tolist())
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; indices per dim "
                         f"{[d[:12] for d in dims]} (counts {[len(d) for d in dims]}); first {i}: got "
                         f"{got[i].item()} want {want[i].item()}")


# ------------------------------------------------------------------ one launch, any epilogue mode
# modes: contig / bias / res (separate residual) / inplace (out aliases res) / f32 / gather (f32 over
# row_idx, the LM head's form) / handoff (in-place residual + hg_out + ssp_out) on plain problems; silu; qkv
PLAIN_BIAS = ("bias", "inplace", "f32", "gather", "handoff")
F32 = ("f32", "gather")


def expected(p: X.Problem, mode: str) -> torch.Tensor:
    e = p.exp
    if mode == "silu":
        return e["out"].double()
    if mode == "qkv":
        return e["q"]
    if mode == "contig":
        return e["prod"]
    if mode == "res":
        want = e["prod"] + p.res.double()
        assert float(want.abs().max()) <= X.BOUND
        return want
    if mode in ("bias", "f32", "gather"):
        return e["biased"]
    return e["full"]


def launch(p: X.Problem, lin: ops.Linear, mode: str, knobs: dict, twice: bool = False) -> dict:
    C = ops.native()
    M, N, K = p.M, p.N, p.K
    epi = 2 if p.kind == "silu" else 3 if p.kind == "qkv" else 1 if mode in F32 else 0
    ncols = N // 2 if p.kind == "silu" else p.qkv["hq"] * 128 if p.kind == "qkv" else N
    strided = mode != "contig"
    kw = dict(ws=ops.workspace(DEV), fault=ops.fault_word(DEV), **knobs)
    if M <= 16:
        kw["sk_ws"] = ops.sk_workspace(DEV)
    if mode == "gather":  # the problem's rows scattered among others
        g = X._gen(M + N + K)
        R = 2 * M + 3
        xs = X.ternary((R, K), 1.0, g).to(BF16)
        idx = torch.randperm(R, generator=g)[:M]
        xs[idx] = p.x
        xg = Guarded(R, K, init=xs)
        kw["row_idx"] = idx.int().to(DEV)
    else:
        xg = Guarded(M, K, init=p.x, strided=strided)
    og = Guarded(M, ncols, torch.float32 if mode in F32 else BF16,
                 init=p.res if mode in ("inplace", "handoff") else None, strided=strided)
    bufs = {"x": xg, "out": og}
    if mode in PLAIN_BIAS or p.kind == "qkv":
        kw["bias"] = lin.bias
    if mode == "res":
        bufs["res"] = Guarded(M, N, init=p.res, pad=40)
        kw["res"] = bufs["res"].view
    elif mode in ("inplace", "handoff"):
        kw["res"] = og.view
    r = {}
    if mode == "handoff":
        g = X._gen(N)
        r["gamma"] = 2.0 ** torch.randint(-1, 2, (N,), generator=g).double()
        bufs["hg"] = Guarded(M, N)
        r["ssp_big"] = torch.full((M * (N // 16) + 128,), X.SENT, dtype=torch.float32, device=DEV)
        kw.update(hg_out=bufs["hg"].view, hg_gamma=r["gamma"].to(BF16).to(DEV),
                  ssp_out=r["ssp_big"][64:64 + M * (N // 16)])
    if p.kind == "qkv":
        m = p.qkv
        kc = torch.full((m["blocks"], m["hkv"], m["bs"], 128), X.SENT, dtype=BF16, device=DEV)
        vc = kc.clone()
        kw.update(positions=m["positions"].to(DEV), slots=m["slots"].to(DEV), cos_sin=m["cos_sin"].to(DEV),
                  k_cache=kc, v_cache=vc, hq=m["hq"], hkv=m["hkv"])
    if p.awq is not None:
        kw.update(awq_scales=lin.scales, awq_zeros=lin.zeros, group=lin.group)
        if lin.szp is not None:
            kw["awq_szp"] = lin.szp

    def go():
        C.gemm(xg.view, lin.wp, N, K, og.view, epi, **kw)

    fault0 = int(ops.fault_word(DEV)[0])
    ents = X.launches(go)
    r["names"], r["blocks"] = [e[0] for e in ents], [e[2] for e in ents]
    what = f"{mode} {knobs} {r['names']}"
    for name, b in bufs.items():
        b.assert_guards(f"{what}: {name}")
    if twice:  # the same workspace again: tickets, granules and slots must have reset themselves
        first = {k: b.big.clone() for k, b in bufs.items()}
        caches = (kc.clone(), vc.clone()) if p.kind == "qkv" else None
        for b in bufs.values():
            b.reset()
        if caches:
            kc.fill_(X.SENT)
            vc.fill_(X.SENT)
        go()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert torch.equal(Guarded._bits(b.big), Guarded._bits(first[k])), f"{what}: second run differs in {k}"
        if caches:
            assert torch.equal(kc, caches[0]) and torch.equal(vc, caches[1]), f"{what}: second run differs in the cache"
    assert int(ops.fault_word(DEV)[0]) == fault0, f"{what}: fault word {int(ops.fault_word(DEV)[0])}"
    r["out"] = og.view.detach().cpu().double()
    if mode == "handoff":
        r["hg"] = bufs["hg"].view.detach().cpu().double()
        ssp = r["ssp_big"].cpu()
        assert bool((ssp[:64] == X.SENT).all()) and bool((ssp[64 + M * (N // 16):] == X.SENT).all()), f"{what}: ssp guards"
        r["ssp"] = ssp[64:64 + M * (N // 16)].double().reshape(M, N // 16)
    if p.kind == "qkv":
        r["k_cache"], r["v_cache"] = kc, vc
    return r


def run_exact(s, mode: str, names: list, twice: bool = False, **knobs) -> dict:
    p, lin = lin_for(s)
    r = launch(p, lin, mode, knobs, twice)
    what = f"{s} {mode} {knobs}"
    assert r["names"] == names, f"{what}: launched {r['names']}, meant {names}"
    want = expected(p, mode)
    assert_exact(r["out"], want, what)
    if mode == "handoff":
        assert_exact(r["hg"], want * r["gamma"][None], what + " hg")
        assert_exact(r["ssp"], want.pow(2).reshape(p.M, p.N // 16, 16).sum(-1), what + " ssp")
    if mode == "qkv":  # written slots, skipped tokens and untouched blocks in one comparison
        assert torch.equal(r["k_cache"].cpu().double(), p.exp["k_cache"]), what + " k_cache"
        assert torch.equal(r["v_cache"].cpu().double(), p.exp["v_cache"]), what + " v_cache"
    return r


def run_sensitive(s, names: list, **knobs) -> None:
    """One weight element (AWQ: one nibble) of the last output column moved by one: the exact
    comparison fails in exactly that column, and the norm-wise statistic of the older tests accepts
    the wrong output."""
    p, _ = lin_for(s)
    n, k = p.N - 1, X.active_k(p, p.K // 2)
    pp = X.perturb(p, n, k)
    r = launch(pp, make_lin(pp), "bias", knobs)
    assert r["names"] == names, (r["names"], names)
    want = expected(p, "bias")
    bad = r["out"] != want
    hit = torch.zeros_like(bad)
    hit[:, n] = p.x[:, k].double() != 0
    assert bool(hit.any()) and torch.equal(bad, hit), f"{s} {knobs}: wrong elements {bad.nonzero()[:8].tolist()}"
    assert X.rel_err(r["out"], want) < 1e-2  # the gap: the old statistic cannot see it


# ------------------------------------------------------------------ the case matrix
Case = namedtuple("Case", "id N K knobs names declined tile")
TILE_NAME = {"f32": "gemm_f32", "gather": "gemm_f32", "silu": "gemm_gate_up", "qkv": "gemm_qkv"}


def tile_name(mode: str) -> str:
    """The decode / K-split tile kernels (gemm_decode.h launch_one), named per epilogue."""
    return TILE_NAME.get(mode, "gemm")


def case(id, N, K, names=None, declined=False, tile=None, **knobs):
    """names: the launches the case means to hit; declined: the family does not take this N (the test
    then asserts the fallback's name instead); tile: the (BM, BN) block tile of a prefill tile code."""
    return Case(id, N, K, knobs, names, declined, tile)


def takes(c, mode: str, heads_only: bool = False) -> bool:
    """The QKV problem brings its own N (whole heads of 128: 512 unless the case's N is one of
    QKV_HEADS), so it skips the cases that are about an N a family declines."""
    return mode != "qkv" or (not c.declined and (not heads_only or c.N in QKV_HEADS))


def pairs(cases, modes, heads_only: bool = False):
    return [pytest.param(c, m, id=f"{c.id}-{m}") for c in cases for m in modes if takes(c, m, heads_only)]


def register(cases, ms, modes, awq=False, heads_only=False):
    for c in cases:
        for M in ms:
            for mode in modes:
                if takes(c, mode, heads_only):
                    spec_for(mode, M, c.N, c.K, awq)


def is_twice(knobs) -> bool:
    return knobs.get("splitk", 0) > 1 or knobs.get("path", 0) == 3


DEC_M = [1, 5, 8, 9, 16]      # XP switches at 4 / 8, the tile is 16 rows
MID_M = [17, 33, 64]
PRE_M = [128, 129, 200]       # 129 / 200: a partial last m-tile
ODD_N = 16 * 37               # a multiple of 16, of no family's block width

# ---- decode tile kernels (gemm_decode.h gemm_kernel<MB = 1>; smallest shape 1 x 256 x 512)
DEC_MODES = ["contig", "bias", "res", "inplace", "f32", "gather", "handoff", "silu", "qkv"]
DEC_CASES = [
    case("auto", 256, 512),
    case("w4s3", ODD_N, 1536, waves=4, splitk=3),
    case("w2s8", 256, 1536, waves=2, splitk=8),
    case("w8s3_k2048", ODD_N, 2048, waves=8, splitk=3),
    case("s2_granules", 256, 512, waves=4, splitk=2),
    case("ntb2", 256, 1536, waves=4, splitk=3, ntb=2),
    case("ntb4", 256, 1536, waves=2, splitk=1, ntb=4),
    # declined: two tiles per block do not divide 37 tiles -> one tile per block (same name)
    case("ntb2_odd", ODD_N, 512, waves=4, splitk=1, ntb=2, declined=True),
]
register(DEC_CASES, DEC_M, DEC_MODES)


@pytest.mark.parametrize("c,mode", pairs(DEC_CASES, DEC_MODES))
@pytest.mark.parametrize("M", DEC_M)
def test_decode_tile(M, c, mode):
    """gemm / gemm_f32 / gemm_gate_up / gemm_qkv at M <= 16 (one-tile and 2 / 4-tile blocks, forced waves
    and K slices, the two-slice granule combine). ntb2_odd: the launcher used to run 2-tile blocks over
    37 tiles and leave the last 16 columns unwritten; it now keeps one tile per block."""
    run_exact(spec_for(mode, M, c.N, c.K), mode, [tile_name(mode)], twice=is_twice(c.knobs), **c.knobs)


def test_row_gather_needs_the_f32_epilogue():
    """The decode kernels load row_idx under the f32 epilogue only (gemm_epilogue.h row_of_e): a bf16
    launch with row_idx used to compute on the ungathered rows 0..M-1; the binding now rejects it."""
    p, lin = lin_for(spec_for("gather", 5, 256, 512))
    x = torch.zeros(13, 512, dtype=BF16, device=DEV)
    out = torch.zeros(5, 256, dtype=BF16, device=DEV)
    idx = torch.arange(5, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="row_idx"):
        ops.native().gemm(x, lin.wp, 256, 512, out, 0, row_idx=idx, ws=ops.workspace(DEV))


# ---- the same kernels at 16 < M (MB = 2 / 4) and the N-split tile kernels (waves -1 / -2)
TILE_MODES = ["bias", "res", "inplace", "f32", "gather", "silu", "qkv"]
MB_CASES = [
    case("auto", 256, 512),
    case("w4s3", ODD_N, 1536, waves=4, splitk=3),
    case("w2s8_k2048", 256, 2048, waves=2, splitk=8),
    case("tile", 256, 512, names=["gemm_tile"], waves=-1),
    case("tile_k1536", 512, 1536, names=["gemm_tile"], waves=-1),
    case("tile3", 256, 512, names=["gemm_tile3"], waves=-2),
    case("tile3_k2048", 512, 2048, names=["gemm_tile3"], waves=-2),
    # declined: 37 tiles are no multiple of the 4 waves of a tile block -> the K-split kernel
    case("tile_odd", ODD_N, 512, waves=-1, declined=True),
]
register(MB_CASES, MID_M + [129], TILE_MODES)


@pytest.mark.parametrize("c,mode", pairs(MB_CASES, TILE_MODES))
@pytest.mark.parametrize("M", MID_M + [129])
def test_tile_kernels(M, c, mode):
    """gemm (MB = 2 / 4 rows of tiles per block) and gemm_tile / gemm_tile3 (64-row blocks: 64 | 65 is
    the row-tile edge, 129 leaves one row in the last block)."""
    names = c.names if c.names else [tile_name(mode)]
    if M >= 128 and not c.knobs:  # path 0 at M >= 128 is the prefill kernel's; it declines a row gather
        names = ["gemm_tile"] if mode == "gather" else ["gemm_prefill", "prefill_reduce"]
    run_exact(spec_for(mode, M, c.N, c.K), mode, names, twice=is_twice(c.knobs), **c.knobs)


# ---- register-stationary decode kernels (gemm_kx.h), bf16: path = 4
KX_MODES = ["bias", "res", "inplace", "handoff", "silu", "qkv", "f32", "gather"]
KX_CASES = [
    case("auto", 256, 512, names=["kx"], path=4),
    case("s3", ODD_N, 1536, names=["kx"], path=4, ntb=-12, splitk=3),
    case("s8", 256, 1536, names=["kx"], path=4, ntb=-12, splitk=8),
    case("s3_k2048", 256, 2048, names=["kx"], path=4, ntb=-12, splitk=3),
    case("s2_granules", 256, 512, names=["kx"], path=4, ntb=-12, splitk=2),
    case("tb2", 256, 1536, names=["kx"], path=4, ntb=-13, splitk=3),
    case("tb4", 256, 1536, names=["kx"], path=4, ntb=-14, splitk=3),
    # declined: 2-tile blocks over 37 tiles -> the tile kernels with their own heuristic
    case("tb2_odd", ODD_N, 512, path=4, ntb=-13, declined=True),
]
# the one-block-per-CU form needs a tile per CU: N = 16 x 256 is its smallest shape on 256 CUs
KX_WIDE = [
    case("wide", 4096, 512, names=["kx_wide"], path=4),
    case("wide_2tiles", 4096 + 16, 512, names=["kx_wide"], path=4),
]
register(KX_CASES, DEC_M, KX_MODES)
register(KX_WIDE, [5, 16], ["bias", "inplace", "handoff", "silu"])


def kx_names(c, mode, awq=False):
    """The f32 epilogue (with or without a row gather) is not taken by the register-stationary kernels."""
    fallback = ["awq_gemm"] if awq else [tile_name(mode)]
    if c.declined or mode in ("f32", "gather"):
        return fallback
    return c.names  # (QKV blocks hold one tile whatever ntb asks)


@pytest.mark.parametrize("c,mode", pairs(KX_CASES, KX_MODES))
@pytest.mark.parametrize("M", DEC_M)
def test_dense_kx(M, c, mode):
    """kx: GROUP blocks of 1 / 2 / 4 tiles, K slices through slabs + tickets or (2 slices) granules.
    Declined and asserted as such: f32, row gather, a tile count the block does not divide."""
    run_exact(spec_for(mode, M, c.N, c.K), mode, kx_names(c, mode), twice=is_twice(c.knobs), **c.knobs)


@pytest.mark.parametrize("c,mode", pairs(KX_WIDE, ["bias", "inplace", "handoff", "silu"]))
@pytest.mark.parametrize("M", [5, 16])
def test_dense_kx_wide(M, c, mode):
    """kx_wide takes N >= 16 tiles x CUs only, so N = 4096 (and 4096 + 16: two tiles on one block)."""
    run_exact(spec_for(mode, M, c.N, c.K), mode, c.names, **c.knobs)


# ---- AWQ decode: awq_kx / awq_kx_wide (path 0, ntb 0 or -12 / -13 / -14) and the K-split awq_gemm (ntb -2)
AWQ_MODES = ["bias", "res", "inplace", "handoff", "silu", "qkv", "f32"]
AWQ_CASES = [
    case("auto", 256, 512, names=["awq_kx"]),
    case("s3", ODD_N, 1536, names=["awq_kx"], ntb=-12, splitk=3),
    case("s8", 256, 1536, names=["awq_kx"], ntb=-12, splitk=8),
    case("s3_k2048", 256, 2048, names=["awq_kx"], ntb=-12, splitk=3),
    case("s2_granules", 256, 512, names=["awq_kx"], ntb=-12, splitk=2),
    case("tb2", 256, 1536, names=["awq_kx"], ntb=-13, splitk=3),
    case("tb4", 256, 1536, names=["awq_kx"], ntb=-14, splitk=3),
    case("tb2_odd", ODD_N, 512, ntb=-13, declined=True),
    case("ksplit", 256, 512, names=["awq_gemm"], ntb=-2, waves=4),
    case("ksplit_s3", ODD_N, 1536, names=["awq_gemm"], ntb=-2, waves=4, splitk=3),
    case("ksplit_s8_k2048", 256, 2048, names=["awq_gemm"], ntb=-2, waves=2, splitk=8),
    case("ksplit_ntb2_odd", ODD_N, 512, names=["awq_gemm"], ntb=2, waves=4),
]
AWQ_WIDE = [
    case("wide", 4096, 512, names=["awq_kx_wide"]),
    case("wide_2tiles", 4096 + 16, 512, names=["awq_kx_wide"]),
]
register(AWQ_CASES, DEC_M, AWQ_MODES, awq=True)
register(AWQ_WIDE, [5, 16], ["bias", "inplace", "handoff", "silu"], awq=True)
spec_for("bias", 8, 256, 512, True, 64)


@pytest.mark.parametrize("c,mode", pairs(AWQ_CASES, AWQ_MODES))
@pytest.mark.parametrize("M", DEC_M)
def test_awq_decode(M, c, mode):
    """awq_kx (register-stationary int4) and awq_gemm (K-split int4). f32 falls back to awq_gemm."""
    run_exact(spec_for(mode, M, c.N, c.K, awq=True), mode, kx_names(c, mode, awq=True), twice=is_twice(c.knobs),
              **c.knobs)


@pytest.mark.parametrize("c,mode", pairs(AWQ_WIDE, ["bias", "inplace", "handoff", "silu"]))
@pytest.mark.parametrize("M", [5, 16])
def test_awq_kx_wide(M, c, mode):
    """awq_kx_wide: one block per CU, N >= 4096 on 256 CUs (the only shapes it takes)."""
    run_exact(spec_for(mode, M, c.N, c.K, awq=True), mode, c.names, **c.knobs)


def test_awq_group64_declined():
    """Group 64 has no packed (scale, zero) operand: the register-stationary kernel declines it."""
    run_exact(spec_for("bias", 8, 256, 512, True, 64), "bias", ["awq_gemm"])


# ---- stream-K decode kernel (gemm_streamk.hip): path = 3
SK_MODES = ["bias", "res", "inplace", "f32", "silu", "qkv", "handoff"]
SK_CASES = [
    case("auto", 1024, 512, path=3),
    case("odd_k1536", ODD_N, 1536, path=3),
    case("k2048", 256, 2048, path=3),
    case("w4", 1024, 512, path=3, waves=4),
    case("u4", ODD_N, 1536, path=3, ntb=4),
    case("two_per_cu", ODD_N, 1536, path=3, splitk=2),
]
register(SK_CASES, DEC_M, SK_MODES)


def sk_names(c, mode, M, N):
    """launch_gemm_sk: SiLU / QKV only with the folded-norm row scale (not exact, not here), no RMSNorm
    hand-off producer; the packed stream must give every block at least one (tile, packed k-step) unit."""
    if mode in ("silu", "qkv", "handoff"):
        return [tile_name(mode)]
    KT = c.K // 32
    xp = 4 if M <= 4 and KT % 4 == 0 else 2 if M <= 8 and KT % 2 == 0 else 1
    G = torch.cuda.get_device_properties(0).multi_processor_count * (2 if c.knobs.get("splitk") == 2 else 1)
    if (N // 16) * (KT // xp) < G:
        return [tile_name(mode)]
    return ["gemm_sk_f32" if mode == "f32" else "gemm_sk_down" if c.K > N else "gemm_sk_o"]


@pytest.mark.parametrize("c,mode", pairs(SK_CASES, SK_MODES))
@pytest.mark.parametrize("M", DEC_M)
def test_streamk(M, c, mode):
    """gemm_sk_*: every case twice on the same publisher slots (they must clear themselves), fault word
    clear. Declined and asserted: SiLU / QKV without the row scale, the hand-off producer, streams
    shorter than the grid."""
    s = spec_for(mode, M, c.N, c.K)
    run_exact(s, mode, sk_names(c, mode, M, build(s).N), twice=True, **c.knobs)


# ---- medium-M kernels (gemm_mid.hip): path = 2
MID_MODES = ["bias", "res", "inplace", "f32", "silu", "qkv", "gather"]
MID_CASES = [
    case("w4", 256, 512, names=["gemm_mid"], path=2, waves=4, splitk=1),
    case("w1s3", ODD_N, 1536, names=["gemm_mid", "prefill_reduce"], path=2, waves=1, splitk=3),
    case("w2s8", 256, 1536, names=["gemm_mid", "prefill_reduce"], path=2, waves=2, splitk=8),
    case("w4s3_k2048", 256, 2048, names=["gemm_mid", "prefill_reduce"], path=2, waves=4, splitk=3),
    # declined: 4-tile blocks over 37 tiles
    case("w4_odd", ODD_N, 512, path=2, waves=4, splitk=1, declined=True),
    case("wide", 256, 512, names=["gemm_midw"], path=2, waves=8),
    case("wide_odd_k1536", ODD_N, 1536, names=["gemm_midw"], path=2, waves=8),
]
register(MID_CASES, MID_M, MID_MODES)
register(MID_CASES[-2:], [8, 16], ["bias", "inplace", "handoff"])


def mid_names(c, mode):
    if c.declined or mode == "gather":
        return [tile_name(mode)]
    return c.names


@pytest.mark.parametrize("c,mode", pairs(MID_CASES, MID_MODES))
@pytest.mark.parametrize("M", MID_M)
def test_mid(M, c, mode):
    """gemm_mid (W tiles per block x K slices + prefill_reduce) and gemm_midw (one block per CU).
    Declined and asserted: a row gather, a tile count W does not divide."""
    run_exact(spec_for(mode, M, c.N, c.K), mode, mid_names(c, mode), twice=is_twice(c.knobs), **c.knobs)


@pytest.mark.parametrize("c,mode", pairs(MID_CASES[-2:], ["bias", "inplace", "handoff"]))
@pytest.mark.parametrize("M", [8, 16])
def test_midw_decode_rows(M, c, mode):
    """gemm_midw also takes decode batches. It has no RMSNorm hand-off epilogue: it used to take such a
    launch and leave hg_out / ssp_out unwritten; it now declines and the decode kernel runs it."""
    run_exact(spec_for(mode, M, c.N, c.K), mode, ["gemm"] if mode == "handoff" else c.names, **c.knobs)


def test_prefill_declines_handoff():
    """path = 1 at decode rows: the prefill kernel has no hand-off epilogue either (same fix)."""
    run_exact(spec_for("handoff", 8, 256, 512), "handoff", ["gemm"], path=1, ntb=64, splitk=1)


# ---- AWQ medium kernel (gemm_awq_mid.hip): path = 2
AMID_MODES = ["bias", "res", "inplace", "f32", "silu", "qkv"]
AMID_CASES = [
    case("w4", 256, 512, names=["awq_mid"], path=2, waves=4, splitk=1),
    case("w1s3", ODD_N, 1536, names=["awq_mid", "prefill_reduce"], path=2, waves=1, splitk=3),
    case("w2s8", 256, 1536, names=["awq_mid", "prefill_reduce"], path=2, waves=2, splitk=8),
    case("w4s3_k2048", 256, 2048, names=["awq_mid", "prefill_reduce"], path=2, waves=4, splitk=3),
    case("w4_odd", ODD_N, 512, path=2, waves=4, splitk=1, declined=True),
    # declined: the wide form (waves = 8) needs a tile per CU
    case("wide_small", 256, 512, path=2, waves=8, declined=True),
]
AMID_WIDE = [case("wide", 4096, 512, names=["awq_mid_wide"], path=2, waves=8),
             case("wide_auto_2tiles", 4096 + 16, 512, names=["awq_mid_wide"], path=2)]
register(AMID_CASES, MID_M, AMID_MODES, awq=True)
register(AMID_WIDE, [17, 64], ["bias", "inplace", "silu"], awq=True)
register(AMID_CASES[:2], [8], ["bias", "handoff"], awq=True)


@pytest.mark.parametrize("c,mode", pairs(AMID_CASES, AMID_MODES))
@pytest.mark.parametrize("M", MID_M)
def test_awq_mid(M, c, mode):
    """awq_mid (+ prefill_reduce under a K split); declined shapes run awq_gemm."""
    names = ["awq_gemm"] if c.declined else c.names
    run_exact(spec_for(mode, M, c.N, c.K, awq=True), mode, names, twice=is_twice(c.knobs), **c.knobs)


@pytest.mark.parametrize("c,mode", pairs(AMID_WIDE, ["bias", "inplace", "silu"]))
@pytest.mark.parametrize("M", [17, 64])
def test_awq_mid_wide(M, c, mode):
    """awq_mid_wide: one block per CU owning whole tiles, N >= 4096 on 256 CUs (its only shapes)."""
    run_exact(spec_for(mode, M, c.N, c.K, awq=True), mode, c.names, **c.knobs)


@pytest.mark.parametrize("c,mode", pairs(AMID_CASES[:2], ["bias", "handoff"]))
def test_awq_mid_decode_rows(c, mode):
    """awq_mid on a decode batch, hand-off producer included (it has that epilogue)."""
    run_exact(spec_for(mode, 8, c.N, c.K, awq=True), mode, c.names, twice=is_twice(c.knobs), **c.knobs)


# ---- LDS-tiled prefill kernels (gemm_prefill.hip): path = 1, ntb = tile code, splitk = K slices
PRE_MODES = ["bias", "res", "inplace", "f32", "silu", "qkv"]
RED = "prefill_reduce"
PRE_CASES = [
    case("auto", 512, 512, names=["gemm_prefill", RED], path=1),
    case("t64", 512, 512, names=["gemm_prefill"], tile=(128, 64), path=1, ntb=64, splitk=1),
    case("t64_s3", 576, 1536, names=["gemm_prefill", RED], tile=(128, 64), path=1, ntb=64, splitk=3),
    case("t128", 512, 512, names=["gemm_prefill"], tile=(128, 128), path=1, ntb=128, splitk=1),
    case("t128_n576", 576, 512, names=["gemm_prefill"], tile=(128, 64), path=1, ntb=128, splitk=1),  # (runs 128 x 64 tiles)
    case("t256_s3", 512, 1536, names=["gemm_prefill2", RED], tile=(256, 128), path=1, ntb=256, splitk=3),
    case("t256_s3_k2048", 512, 2048, names=["gemm_prefill2", RED], tile=(256, 128), path=1, ntb=256, splitk=3),
    # declined: N = 576 is no multiple of 128 -> the K-split tile kernel; N = 16 x 37 of no tile at all
    case("t256_n576", 576, 512, path=1, ntb=256, splitk=1, declined=True),
    case("t64_odd", ODD_N, 512, path=1, ntb=64, splitk=1, declined=True),
    case("t512", 512, 512, names=["gemm_prefill2"], tile=(256, 256), path=1, ntb=512, splitk=1),
    case("t1024", 512, 512, names=["gemm_prefill4"], tile=(256, 256), path=1, ntb=1024, splitk=1),
    case("t1024_s3", 512, 1536, names=["gemm_prefill4", RED], tile=(256, 256), path=1, ntb=1024, splitk=3),
    case("t768", 640, 512, names=["gemm_prefill4"], tile=(256, 128), path=1, ntb=768, splitk=1),
    case("t1025_tail", 512, 512, names=["gemm_prefill4sk"], tile=(256, 256), path=1, ntb=1025),
    case("t769_tail_k2048", 640, 2048, names=["gemm_prefill4sk"], tile=(256, 128), path=1, ntb=769),
    case("t1280", 512, 512, names=["gemm_prefill2"], tile=(128, 128), path=1, ntb=1280, splitk=1),
    case("t1281_s2_k2048", 512, 2048, names=["gemm_prefill2", RED], tile=(128, 128), path=1, ntb=1281, splitk=2),
    case("t640", 576, 512, names=["gemm_prefill2"], tile=(128, 64), path=1, ntb=640, splitk=1),
    case("t641", 576, 512, names=["gemm_prefill2"], tile=(128, 64), path=1, ntb=641, splitk=1),
    case("t2560", 512, 512, names=["gemm_prefill2"], tile=(64, 512), path=1, ntb=2560, splitk=1),
    case("t2561", 640, 512, names=["gemm_prefill2"], tile=(128, 320), path=1, ntb=2561, splitk=1),
]
register(PRE_CASES, PRE_M, PRE_MODES, heads_only=True)


@pytest.mark.parametrize("c,mode", pairs(PRE_CASES, PRE_MODES, heads_only=True))
@pytest.mark.parametrize("M", PRE_M)
def test_prefill(M, c, mode):
    """gemm_prefill / gemm_prefill2 / gemm_prefill4 / gemm_prefill4sk (+ prefill_reduce under a forced K
    split); 129 and 200 rows leave a partial last m-tile of every tile height (64 / 128 / 256). The name
    alone cannot tell the tile codes of one kernel apart (gemm_prefill2 has seven geometries): a forced
    code's grid must be ceil(M / BM) * (N / BN) tiles times the forced K slices, the persistent kernel's
    one block per CU."""
    names = [tile_name(mode)] if c.declined else c.names
    twice = is_twice(c.knobs) or "4sk" in names[0] or RED in names
    s = spec_for(mode, M, c.N, c.K)
    r = run_exact(s, mode, names, twice=twice, **c.knobs)
    if c.tile is not None:
        bm, bn = c.tile
        nz = max(c.knobs.get("splitk", 0), 1)
        want = (torch.cuda.get_device_properties(0).multi_processor_count if "4sk" in names[0]
                else -(-M // bm) * (lin_for(s)[0].N // bn) * nz)
        assert r["blocks"][0] == want, (f"{c.id} {mode} M={M}: {names[0]} ran {r['blocks'][0]} blocks, "
                                        f"tile {c.tile} x {nz} slices means {want}")


# ---- one sensitivity case per family
SENS = [
    ("dense", 8, 256, 512, ["gemm"], dict(waves=4, splitk=2)),
    ("dense", 33, ODD_N, 1536, ["gemm"], dict(waves=4, splitk=3)),
    ("dense", 64, 256, 512, ["gemm_tile"], dict(waves=-1)),
    ("dense", 33, 256, 512, ["gemm_tile3"], dict(waves=-2)),
    ("dense", 8, ODD_N, 1536, ["kx"], dict(path=4, ntb=-12, splitk=3)),
    ("dense", 5, 4096 + 16, 512, ["kx_wide"], dict(path=4)),
    ("awq", 8, ODD_N, 1536, ["awq_kx"], dict(ntb=-12, splitk=3)),
    ("awq", 5, 4096 + 16, 512, ["awq_kx_wide"], dict()),
    ("awq", 8, ODD_N, 1536, ["awq_gemm"], dict(ntb=-2, waves=4, splitk=3)),
    ("dense", 8, ODD_N, 1536, ["gemm_sk_down"], dict(path=3)),
    ("dense", 33, ODD_N, 1536, ["gemm_mid", RED], dict(path=2, waves=1, splitk=3)),
    ("dense", 33, 256, 512, ["gemm_midw"], dict(path=2, waves=8)),
    ("awq", 33, ODD_N, 1536, ["awq_mid", RED], dict(path=2, waves=1, splitk=3)),
    ("awq", 17, 4096, 512, ["awq_mid_wide"], dict(path=2, waves=8)),
    ("dense", 129, 576, 1536, ["gemm_prefill", RED], dict(path=1, ntb=64, splitk=3)),
    ("dense", 129, 512, 1536, ["gemm_prefill2", RED], dict(path=1, ntb=256, splitk=3)),
    ("dense", 129, 512, 512, ["gemm_prefill4"], dict(path=1, ntb=1024, splitk=1)),
    ("dense", 129, 512, 512, ["gemm_prefill4sk"], dict(path=1, ntb=1025)),
]
for _k, _M, _N, _K, _n, _kw in SENS:
    spec_for("bias", _M, _N, _K, _k == "awq")


@pytest.mark.parametrize("kind,M,N,K,names,knobs", SENS, ids=[f"{s[4][0]}-{s[1]}" for s in SENS])
def test_one_wrong_weight_is_seen(kind, M, N, K, names, knobs):
    run_sensitive(spec_for("bias", M, N, K, kind == "awq"), names, **knobs)


# ---- awq_dequant: packed int4 -> packed bf16
@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("N,K,group", [(256, 512, 128), (ODD_N, 1536, 128), (256, 512, 64)])
def test_awq_dequant_exact(N, K, group, gamma):
    """The dequantised matrix, element for element (with a power-of-two gamma folded in), in the
    packed order ops.unpack_weight undoes; nothing past N * K elements is written."""
    p, lin = lin_for(spec_for("bias", 8, N, K, True, group))
    out = torch.full((N * K + 256,), X.SENT, dtype=BF16, device=DEV)
    g = None
    want = p.w.double()
    if gamma:
        g = 2.0 ** torch.randint(-1, 2, (K,), generator=X._gen(K)).double()
        want = want * g[None]
        g = g.to(BF16).to(DEV)
    ops.native().awq_dequant(lin.wp, lin.scales, lin.zeros, N, K, group, out, g)
    torch.cuda.synchronize()
    assert_exact(ops.unpack_weight(out[:N * K], N, K), want, "awq_dequant")
    assert bool((out[N * K:] == X.SENT).all())
